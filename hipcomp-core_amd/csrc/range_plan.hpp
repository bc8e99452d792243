// range_plan.hpp -- the plan of a ranged read of a container (hlif.hip, decompress_range): which chunks bytes
// [first_byte, first_byte + num_bytes) of the uncompressed buffer touch, which of them are decoded into a scratch
// slot (EDGE chunks: only partly inside the range, or landing in `out` where the decoder's alignment contract does
// not hold) and which straight into the caller's `out` (INTERIOR chunks), the byte span every chunk contributes
// and where it lands, and how the chunks fall into passes.
//
// Pure arithmetic in constexpr functions: standard headers only, no HIP, no state.  The host plans with
// range_plan(); the kernels of range_kernels.hip get the plan as an argument and ask range_span() per chunk, so
// both sides compute one thing.  tests/test_range_plan_cpu.py compiles this header with g++ alone
// (tests/range_plan_driver.cpp prints it) and compares it with a restatement.  Sizes up to 2^63 do not overflow.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace range {

struct Plan
{
  uint64_t decomp_bytes = 0, chunk_bytes = 0;
  uint64_t first_byte = 0, num_bytes = 0;
  uint64_t first_chunk = 0; // the chunks touched: [first_chunk, first_chunk + chunks)
  uint64_t chunks = 0;
  // 0: the interior chunks land aligned and go straight into `out`; the only edge chunks are the first and the
  //    last one touched, where the range cuts them (slots 0 and 1)
  // 1: an interior chunk would land off the decoder's alignment: every chunk is an edge chunk (slot = its
  //    position in its pass)
  uint32_t all_edge = 0;
  uint32_t per_pass = 0;    // chunks of a pass, the last one may be shorter
  uint64_t passes = 0;
};

struct Span
{
  uint64_t src_at = 0; // first wanted byte, from the chunk's start
  uint64_t dst_at = 0; // where it lands, from out
  uint64_t bytes = 0;  // how many (0 < bytes <= cap)
  uint64_t cap = 0;    // bytes of the whole chunk
  bool edge = false;   // decoded into slot `slot`, src_at .. src_at + bytes copied to out + dst_at
  uint32_t slot = 0;
};

// slots a pass may need: 2, or per_pass where all_edge
constexpr uint32_t kTwoEdges = 2;

// false: the range is refused (hipcompErrorInvalidValue) -- it overflows, reaches past decomp_bytes, or is not made
// of whole elements.  `slab`: chunks a pass's lists hold (>= 1); `edge_slots`: scratch slots there are (>= 2);
// `align` (a power of two, >= 1): what the decoder asks of an output pointer; `out_mod`: the address of `out`
// modulo align; `elem`: the element size first_byte and num_bytes must be multiples of (1: any).
constexpr bool range_plan(Plan& p, uint64_t decomp_bytes, uint64_t chunk_bytes, uint64_t first_byte, uint64_t num_bytes,
                          uint32_t slab, uint32_t edge_slots, uint32_t align, uint32_t out_mod, uint32_t elem)
{
  p = Plan();
  p.decomp_bytes = decomp_bytes;
  p.chunk_bytes = chunk_bytes;
  p.first_byte = first_byte;
  p.num_bytes = num_bytes;
  if (chunk_bytes == 0 || slab == 0 || edge_slots < kTwoEdges || align == 0 || elem == 0)
    return false;
  if (first_byte > decomp_bytes || num_bytes > decomp_bytes - first_byte) // (first_byte + num_bytes may wrap)
    return false;
  if (first_byte % elem || num_bytes % elem)
    return false;
  if (num_bytes == 0)
    return true;
  const uint64_t end = first_byte + num_bytes; // <= decomp_bytes
  p.first_chunk = first_byte / chunk_bytes;
  const uint64_t last_chunk = (end - 1) / chunk_bytes;
  p.chunks = last_chunk - p.first_chunk + 1;
  // interior chunks: those wholly inside the range.  Chunk c lands at out + c * chunk_bytes - first_byte; the
  // residues modulo align repeat after at most align chunks.
  const uint64_t lo = p.first_chunk + (first_byte % chunk_bytes ? 1 : 0);
  uint64_t hi = last_chunk + 1; // interior: [lo, hi)
  {
    const uint64_t last_start = last_chunk * chunk_bytes;
    const uint64_t last_cap = decomp_bytes - last_start < chunk_bytes ? decomp_bytes - last_start : chunk_bytes;
    if (end - last_start != last_cap)
      hi = last_chunk;
  }
  for (uint64_t c = lo, k = 0; c < hi && k < align; ++c, ++k)
    if ((out_mod + (c * chunk_bytes - first_byte)) % align)
      p.all_edge = 1;
  p.per_pass = p.all_edge && edge_slots < slab ? edge_slots : slab;
  p.passes = (p.chunks + p.per_pass - 1) / p.per_pass;
  return true;
}

// the chunks of pass k: [pass_first, pass_first + pass_count)
constexpr uint64_t range_pass_first(const Plan& p, uint64_t k) { return p.first_chunk + k * p.per_pass; }
constexpr uint32_t range_pass_count(const Plan& p, uint64_t k)
{
  const uint64_t left = p.chunks - k * p.per_pass;
  return (uint32_t)(left < p.per_pass ? left : p.per_pass);
}

// what chunk c (one of the plan's) contributes; pass_first: the first chunk of c's pass
constexpr Span range_span(const Plan& p, uint64_t c, uint64_t pass_first)
{
  Span s;
  const uint64_t start = c * p.chunk_bytes;
  s.cap = p.decomp_bytes - start < p.chunk_bytes ? p.decomp_bytes - start : p.chunk_bytes;
  const uint64_t from = start > p.first_byte ? start : p.first_byte;
  const uint64_t range_end = p.first_byte + p.num_bytes, chunk_end = start + s.cap;
  const uint64_t to = chunk_end < range_end ? chunk_end : range_end;
  s.src_at = from - start;
  s.dst_at = from - p.first_byte;
  s.bytes = to - from;
  s.edge = p.all_edge || s.bytes != s.cap;
  s.slot = p.all_edge ? (uint32_t)(c - pass_first) : (c == p.first_chunk ? 0u : 1u);
  return s;
}

} // namespace range
} // namespace hcamd
