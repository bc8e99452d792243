// lz4_constants.hpp -- what the LZ4 kernels (lz4_kernels.hip) and their launch plan (lz4_plan.cpp) both
// build on, stated once.  Standard headers only: the plan is compiled and tested without HIP.
#pragma once

#include <cstdint>

namespace hcamd {

// Classes = launch shapes of the compressor (lz4_common.hiph, above work lists; only speed depends on the
// class, never the bytes):
//   kClassMix     tables in LDS, tags, the walk: data with match-less stretches
//   kClassDense   far / both kernels, lean form, widest span, all 32 waves per CU
//   kClassSparse  the same kernels with fewer device-table waves per CU (text: the
//                 table probes of those waves are what the fabric limits)
//   kClassWide    the wide form (run-length data)
constexpr uint32_t kClassMix = 0, kClassDense = 1, kClassSparse = 2, kClassWide = 3, kNumClasses = 4;

// The header of the compress temp buffer (words, lz4_far.hiph, lz4_route_kernel): [0..3] ticket counters,
// [4..7] list lengths, [8..10] totals of the sample counters {repeats, looked, near} (for tests and
// measurements), [12] the length of the list of chunks the far kernels gave back to the LDS shape
// (give_away), [13] the ticket counter of the launch that works through it.
constexpr uint32_t kHeaderWords = 64;
constexpr uint32_t kHeaderRetryCount = 12, kHeaderRetryTicket = 13;

// The routing kernel: waves per workgroup, most chunks one workgroup routes.
constexpr int kRouteWaves = 4;
constexpr uint32_t kRouteMostPerGroup = 64;

// Most waves (= chunks in flight) one compression workgroup of the "mix" shape
// holds.  Four (one per SIMD): the kernel may then use up to 256 vector
// registers and keeps clear of the accumulation registers, which its walk uses
// by name (lz4_kernels.hip, HC_WALK_AGPRS; tests/test_build_guards_cpu.py
// checks the build).
constexpr int kLz4MaxWavesPerGroup = 4;

// LDS bytes of the pair kernel's command words in front of its table (lz4_mix.hiph, kPair*)
constexpr uint32_t kPairSyncBytes = 64; // (48 .. 63: the diagnostic build's two sums)

// The far kernel (lz4_far.hiph, lz4_compress_kernel_far): most waves per workgroup, the scratch of a lone
// LDS-table wave (u16 each; 512 per wave in full workgroups), lanes a trip of the lean form looks up.
constexpr int kFarMaxWavesPerGroup = 16;
constexpr uint32_t kFarScratchSlots = 2048;
constexpr int kFarSpan = 40; // (bytes, 20 000 chunks: 32: harness 88 / text 38.5 GB/s, 40: 97 / 38.6, 48: 99.5 / 37.2)
constexpr int kFarSpanFull = 64; // (all lanes: the words behind the window, far_straight_several: `ext`)

// Decoder waves per workgroup (lz4_decode.hiph: why four)
constexpr int kDecompWavesPerBlock = 4;

} // namespace hcamd
