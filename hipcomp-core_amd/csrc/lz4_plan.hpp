// lz4_plan.hpp -- the launch plan of the LZ4 kernels: which kernels lz4_launch_compress /
// lz4_launch_decompress (lz4_kernels.hip) launch, with what grid, workgroup, LDS and arguments, and where
// in the caller's temp buffer.  A pure function of the call's sizes and the device's CU count
// (lz4_plan.cpp: no HIP, no state, no environment; tests/test_lz4_plan_cpu.py pins it).
#pragma once

#include <cstddef>
#include <cstdint>

#include "device_facts.hpp"
#include "lz4_constants.hpp"

namespace hcamd {

enum class Lz4Mode { Auto, Mix, Far, FarSparse, FarWide };

// The measurement knobs (knobs build only: lz4_kernels.hip, lz4_overrides_from_environment); the
// library that ships plans with none.
struct Lz4Overrides
{
  bool has_pair = false;
  int pair = 0;                          // HIPCOMP_LZ4_PAIR: pair mode (below) where ht_size >= 8192
  bool inpos = true;                     // HIPCOMP_LZ4_INPOS=0: 4-byte elements with tag tables
  uint32_t pair_lds = 0;                 // HIPCOMP_LZ4_PAIR_LDS: more LDS per pair (fewer pairs per CU)
  uint32_t near = 0, far = 0, slots = 0; // HIPCOMP_LZ4_GEOMETRY="near,far,slots" (slots 0: not set)
  uint32_t span = 0;                     // HIPCOMP_LZ4_SPAN (0: not set)
};

// The compress temp buffer (the caller's, hipcompBatchedLZ4CompressGetTempSize bytes by contract), in
// this order as far as it goes: the header (kHeaderWords, 4-byte aligned), the routing kernel's class
// lists (kNumClasses x batch words), the retry list (batch words: the chunks the far kernels give back to
// the LDS shape), hash tables for the far kernel's device-table waves (max(ht_size, 8) uint16 each,
// 16-byte aligned).  Byte offsets from the buffer's start; kAbsent: it does not hold that part.
constexpr size_t kAbsent = ~size_t(0);
struct Lz4TempLayout
{
  size_t header, lists, retry, far_tables;
  size_t far_capacity; // tables at far_tables
};
// base_mod16: the buffer's address modulo 16; temp_bytes 0: no buffer
Lz4TempLayout lz4_temp_layout(uint32_t ht_size, size_t batch, unsigned base_mod16, size_t temp_bytes);
// what the layout makes use of at most, wherever the buffer lies (for callers that size their own
// scratch: hlif.hip): the header, the lists, the retry list and min(batch, 8192) tables
size_t lz4_compress_temp_bytes_used(uint32_t ht_size, size_t batch);

// The LDS shape: lz4_compress_kernel_pair (two waves per chunk, one chunk per workgroup: data without
// matches in chunks of 16 .. 64 KiB and batches of several thousand) or lz4_compress_kernel_mix (one chunk
// per wave, up to kLz4MaxWavesPerGroup waves per workgroup).
struct Lz4LdsLaunch
{
  bool pair;
  uint32_t grid, waves, lds_bytes, per_ticket;
  uint32_t pair_tags, table_bytes;                // pair: 0 no tags, 1 a tag table, 2 tags in the positions
  uint32_t tagged, stride_tagged, stride_plain;   // mix: waves with a tag table; LDS bytes of one wave's tables
  bool inpos;                                     // mix: the tags live in the positions (flag 2)
};

// The far kernel for one class: per workgroup `near` waves with their table in LDS and `far` with theirs
// in the temp buffer, `slots` scratch slots per wave; groups == 0: not launched.
struct Lz4FarLaunch
{
  uint32_t groups, near, far, slots, lds_bytes, span, per_ticket;
  uint32_t waves() const { return near + far; }
};

struct Lz4CompressPlan
{
  Lz4TempLayout temp;
  bool refused;      // a placement without the header: its slots are per resident wave (hipErrorInvalidValue)
  bool routed;       // route, the LDS shape (its list), the far classes (theirs), the retry list (if any)
  uint32_t route_grid, route_per_group;
  Lz4LdsLaunch lds;  // not routed: launched unless forced_far is
  Lz4FarLaunch far[kNumClasses]; // [kClassDense .. kClassWide]
  uint32_t forced_far; // not routed: the far class launched instead of the LDS shape, else kClassMix
};
// batch > 0 and < 2^31; cus: compute units of the device; placed: the call places its chunks (placement.hpp)
Lz4CompressPlan lz4_plan_compress(uint32_t ht_size, size_t batch, int elem_size, size_t max_chunk_bytes, Lz4Mode mode,
                                  uint32_t cus, unsigned base_mod16, size_t temp_bytes, bool placed,
                                  const Lz4Overrides& knobs);

// The decoder: `grid` workgroups of kDecompWavesPerBlock waves.  More chunks than the chip holds waves and a
// temp buffer: a persistent grid whose waves draw chunks from ONE word of the buffer as their ticket
// counter, another word for every call (ticket_offset); else (ticket_words == 0) a wave per chunk.
struct Lz4DecompressPlan
{
  uint32_t grid;
  size_t first_word, ticket_words; // byte offset of the buffer's first word, how many there are
  size_t ticket_offset(uint32_t call) const { return first_word + call % ticket_words * sizeof(uint32_t); }
};
Lz4DecompressPlan lz4_plan_decompress(size_t batch, uint32_t cus, unsigned base_mod16, size_t temp_bytes);

} // namespace hcamd
