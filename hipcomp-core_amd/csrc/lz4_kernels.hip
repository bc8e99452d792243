// lz4_kernels.hip -- gfx950 kernels of the batched LZ4 block codec: the one
// translation unit.  The device code lies in the parts included below,
//   lz4_common.hiph  hash, sequence writers, the reference's insert rule, the
//                    one-window match search, match length, emission, tickets
//   lz4_mix.hiph     "mix" shape: hash (+ tag) tables in LDS, block-pipelined walk
//                    over match-less stretches -- data that does not compress
//   lz4_far.hiph     "far" shapes: tables in device memory (the caller's temp
//                    buffer) or LDS, several sequences per trip to memory --
//                    data that compresses; the sampling kernel that picks
//   lz4_decode.hiph  the decoder
// and the host launchers follow here.
//
// Compressed bytes are those of the reference's wave64 encoder
// (reference src/LZ4Kernels.hiph:793-969 compressStream<T>), produced by a
// different mechanism:
//
//   reference                               here
//   --------------------------------------  ---------------------------------
//   32 KiB hash table per chunk in HBM      data without matches: table in LDS
//   (temp space), global_store_short        (ds_read_u16 / ds_write_b16); data
//                                           that compresses: one table per
//                                           RESIDENT WAVE in the temp space
//                                           (32 waves per CU instead of 5)
//   every table candidate is verified by    a second LDS table holds 8 more
//   a 4-byte gather from the input (a       hash bits of the word each entry
//   64-line gather per window: the memory   was made from; a candidate whose
//   pipe's bound, scripts/probes/           tag differs cannot match and is
//   gather_rate.hip)                        not fetched
//   warpMatchAny = 64-step LDS loop, twice  in-window duplicates: found through
//   per window (:218-245)                   the table itself (one-window path:
//                                           lane ids posted in reversed lane
//                                           order; walk: a lane that does not
//                                           read back its own insert shares a
//                                           slot), exact compare only for
//                                           those lanes
//   second warpMatchAny for the insert      insert rule (incl. the wave64
//   (:722-741) + hardware arbitration of    `int` truncation)
//   same-address global_store_short         = ONE masked LDS store with the
//                                           lanes in priority order ("sigma
//                                           order", see sigma_of_lane)
//   one window, one sequence at a time      match-less stretches: blocks of
//   (:925-956)                              windows, all LDS traffic of a block
//                                           issued back to back, decisions one
//                                           block later (walk_*); compressible
//                                           data: one trip to the table and to
//                                           the candidates serves several
//                                           sequences (far_straight_several)
//   shuffleLiterals (:754-791)              one unaligned dword load per lane
//   1 byte/lane literal + match compare     16-byte/lane copies, 4-byte/lane
//                                           match-length compare
//
// One chunk per wavefront: the window loop is a serial dependency chain, the
// 64 lanes are the 64 window positions.
//
// Decoder: reference src/LZ4Kernels.hiph:971-1097 decompressStream.

#include "device_facts.hpp"
#include "lz4_launch.hpp"
#include "placement.hiph"
#include "wave_utils.hpp"


#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>


namespace hcamd {

namespace {

#include "lz4_common.hiph"
#include "lz4_mix.hiph"
#include "lz4_far.hiph"
#include "lz4_decode.hiph"

} // namespace

// ---- launchers: the plan (lz4_plan.cpp) says what; here it is launched -----

namespace {

typedef void (*MixKernel)(
    const uint8_t* const*, const size_t*, uint8_t* const*, size_t*, uint32_t, uint32_t, uint32_t, uint32_t,
    uint32_t, uint32_t*, uint32_t, const uint32_t*, const uint32_t*, Lz4Placement, uint32_t);
typedef void (*FarKernel)(const uint8_t* const*, const size_t*, uint8_t* const*, size_t*, uint32_t, uint16_t*,
                          uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t, uint32_t, const uint32_t*,
                          const uint32_t*, Lz4Placement, uint32_t*, uint32_t*);

typedef void (*PairKernel)(
    const uint8_t* const*, const size_t*, uint8_t* const*, size_t*, uint32_t, uint32_t, uint32_t,
    uint32_t, uint32_t*, uint32_t, const uint32_t*, const uint32_t*, Lz4Placement, uint32_t);

PairKernel pair_kernel_for(int elem_size)
{
  return elem_size == 1 ? lz4_compress_kernel_pair<1> : elem_size == 2 ? lz4_compress_kernel_pair<2>
                                                                      : lz4_compress_kernel_pair<4>;
}

MixKernel mix_kernel_for(int elem_size)
{
  return elem_size == 1 ? lz4_compress_kernel_mix<1> : elem_size == 2 ? lz4_compress_kernel_mix<2>
                                                                      : lz4_compress_kernel_mix<4>;
}
template <int FORM>
FarKernel far_kernel_of_form(int elem_size)
{
  return elem_size == 1 ? lz4_compress_kernel_far<1, FORM> : elem_size == 2 ? lz4_compress_kernel_far<2, FORM>
                                                                             : lz4_compress_kernel_far<4, FORM>;
}
FarKernel far_kernel_for(int elem_size, uint32_t cls)
{
  return cls == kClassWide ? far_kernel_of_form<kFormWide>(elem_size)
         : cls == kClassDense ? far_kernel_of_form<kFormChains>(elem_size) : far_kernel_of_form<kFormLean>(elem_size);
}

// more than 64 KiB of dynamic LDS has to be asked for, once per kernel and device (raise_dynamic_lds_once)
int raise_dynamic_lds_limit()
{
  hipError_t r = hipSuccess;
  for (int es = 1; es <= 4 && r == hipSuccess; es *= 2) {
    r = hipFuncSetAttribute(reinterpret_cast<const void*>(mix_kernel_for(es)),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsPerCu);
    for (uint32_t cls = kClassDense; cls <= kClassWide && r == hipSuccess; ++cls)
      r = hipFuncSetAttribute(reinterpret_cast<const void*>(far_kernel_for(es, cls)),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsPerCu);
  }
  return r;
}

} // namespace

// The library that ships reads nothing from the environment: every chunk goes where the routing
// kernel sends it.  The knobs below exist in the measurement / test build only
// (`make VARIANT=knobs` -> lib/libhipcomp_knobs.so: the same device code, tests/test_build_guards_cpu.py
// compares the code objects), where they are read at every call so that the tests can switch shapes
// inside one process.  HIPCOMP_LZ4_SHAPE = auto | mix | far | fars | farw: the mode (lz4_launch.hpp); the
// others fill the plan's overrides (lz4_plan.hpp, Lz4Overrides).
#ifdef HC_MEASUREMENT_KNOBS
Lz4Mode lz4_mode_from_environment()
{
  const char* e = std::getenv("HIPCOMP_LZ4_SHAPE");
  if (e && std::strcmp(e, "mix") == 0)
    return Lz4Mode::Mix;
  if (e && std::strcmp(e, "far") == 0)
    return Lz4Mode::Far;
  if (e && std::strcmp(e, "fars") == 0)
    return Lz4Mode::FarSparse;
  if (e && std::strcmp(e, "farw") == 0)
    return Lz4Mode::FarWide;
  return Lz4Mode::Auto;
}

namespace {
Lz4Overrides lz4_overrides()
{
  Lz4Overrides o;
  if (const char* e = std::getenv("HIPCOMP_LZ4_PAIR")) {
    o.has_pair = true;
    o.pair = std::atoi(e);
  }
  if (const char* e = std::getenv("HIPCOMP_LZ4_INPOS"))
    o.inpos = std::atoi(e) != 0;
  if (const char* e = std::getenv("HIPCOMP_LZ4_PAIR_LDS"))
    o.pair_lds = (uint32_t)std::atoi(e);
  unsigned a = 0, b = 0, c = 0;
  const char* e = std::getenv("HIPCOMP_LZ4_GEOMETRY");
  if (e && std::sscanf(e, "%u,%u,%u", &a, &b, &c) == 3 && a + b >= 1 && a + b <= (unsigned)kFarMaxWavesPerGroup
      && c >= 64 && c <= 4096 && (c & (c - 1)) == 0) {
    o.near = a;
    o.far = b;
    o.slots = c;
  }
  if (const char* s = std::getenv("HIPCOMP_LZ4_SPAN")) {
    const int v = std::atoi(s);
    if (v >= 8 && v <= 64)
      o.span = (uint32_t)v;
  }
  return o;
}
} // namespace
#else
Lz4Mode lz4_mode_from_environment() { return Lz4Mode::Auto; }

namespace {
Lz4Overrides lz4_overrides() { return Lz4Overrides(); }
} // namespace
#endif

#ifdef HC_PAIR_DEBUG
// (diagnostic build only; the name makes it pass the export map)
extern "C" int hipcompBatchedLZ4DebugPair(uint32_t* host16, int reset)
{
  uint32_t zeros[32] = {};
  if (hipMemcpyFromSymbol(host16, HIP_SYMBOL(g_pair_dbg), sizeof(zeros)) != hipSuccess)
    return 1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_pair_dbg), zeros, sizeof(zeros)) != hipSuccess)
    return 2;
  return 0;
}
#endif

// words[0 .. blockDim.x) = 0: the ticket counters of a call, on its stream
__global__ void lz4_zero_words_kernel(uint32_t* words)
{
  words[threadIdx.x] = 0;
}


size_t lz4_placement_slots()
{
  // (the far kernels: at most 32 waves per CU; the mix kernel 4)
  return (size_t)num_cus_of_current_device() * 32u;
}

hipError_t lz4_launch_compress(
    const uint8_t* const* in_ptrs, const size_t* in_bytes,
    uint8_t* const* out_ptrs, size_t* out_bytes, uint32_t ht_size,
    size_t batch, int elem_size, void* temp, size_t temp_bytes,
    size_t max_chunk_bytes, Lz4Mode mode, hipStream_t stream, const Lz4Placement* place_or_null)
{
  const Lz4Placement place = place_or_null ? *place_or_null : Lz4Placement();
  const Lz4CompressPlan plan = lz4_plan_compress(
      ht_size, batch, elem_size, max_chunk_bytes, mode, (uint32_t)num_cus_of_current_device(),
      (unsigned)(reinterpret_cast<uintptr_t>(temp) & 15u), temp ? temp_bytes : 0, place.slots != nullptr,
      lz4_overrides());
  auto in_temp = [&](size_t offset) {
    return offset == kAbsent ? nullptr : static_cast<uint8_t*>(temp) + offset;
  };
  uint32_t* const header = reinterpret_cast<uint32_t*>(in_temp(plan.temp.header));
  uint32_t* const lists = reinterpret_cast<uint32_t*>(in_temp(plan.temp.lists));
  uint32_t* const retry_list = reinterpret_cast<uint32_t*>(in_temp(plan.temp.retry));
  uint16_t* const far_tables = reinterpret_cast<uint16_t*>(in_temp(plan.temp.far_tables));
  const hipError_t raised = (hipError_t)raise_dynamic_lds_once(raise_dynamic_lds_limit);
  if (raised != hipSuccess)
    return raised;
  if (plan.refused)
    return hipErrorInvalidValue;
  // (`ticket_word`: the header's word that is this launch's ticket counter, none without a header; give: its
  // waves may hand chunks that open like data that compresses on to the sparse class, whose kernel runs behind them)
  auto launch_lds = [&](const uint32_t* count, const uint32_t* list, uint32_t ticket_word, bool give) {
    const Lz4LdsLaunch& l = plan.lds;
    uint32_t* ticket = header ? header + ticket_word : nullptr;
    if (l.pair)
      pair_kernel_for(elem_size)<<<dim3(l.grid), dim3(l.waves * kWave), l.lds_bytes, stream>>>(
          in_ptrs, in_bytes, out_ptrs, out_bytes, ht_size, l.pair_tags, l.table_bytes,
          (uint32_t)batch, ticket, l.per_ticket, count, list, place, give ? 1u : 0u);
    else
      mix_kernel_for(elem_size)<<<dim3(l.grid), dim3(l.waves * kWave), l.lds_bytes, stream>>>(
          in_ptrs, in_bytes, out_ptrs, out_bytes, ht_size, l.tagged, l.stride_tagged, l.stride_plain,
          (uint32_t)batch, ticket, l.per_ticket, count, list, place, (give ? 1u : 0u) | (l.inpos ? 2u : 0u));
  };
  auto launch_far = [&](uint32_t cls, const uint32_t* counts, const uint32_t* all_lists) {
    const Lz4FarLaunch& g = plan.far[cls];
    far_kernel_for(elem_size, cls)<<<dim3(g.groups), dim3(g.waves() * kWave), g.lds_bytes, stream>>>(
        in_ptrs, in_bytes, out_ptrs, out_bytes, ht_size, far_tables, g.near, g.slots, g.span, (uint32_t)batch,
        header + cls, g.per_ticket, cls, counts, all_lists, place,
        counts && retry_list ? header + kHeaderRetryCount : nullptr, counts ? retry_list : nullptr);
  };
  if (!header) { // (a temp buffer too small for a ticket counter)
    launch_lds(nullptr, nullptr, kClassMix, false);
    return hipSuccess;
  }
  // (zeroed by a kernel, not hipMemsetAsync: see lz4_launch_decompress)
  lz4_zero_words_kernel<<<dim3(1), dim3(kHeaderWords), 0, stream>>>(header);
  {
    const hipError_t zeroed = hipGetLastError();
    if (zeroed != hipSuccess)
      return zeroed;
  }
  if (plan.routed) {
    // every chunk to the shape its data calls for
    lz4_route_kernel<<<dim3(plan.route_grid), dim3(kRouteWaves * kWave), 0, stream>>>(
        in_ptrs, in_bytes, (uint32_t)batch, plan.route_per_group, header, lists);
    launch_lds(header + 4 + kClassMix, lists + kClassMix * batch, kClassMix, true);
    for (uint32_t cls = kClassDense; cls <= kClassWide; ++cls) {
      if (plan.far[cls].groups == 0)
        return hipErrorInvalidValue; // (cannot happen: the LDS-table waves need nothing but the header)
      launch_far(cls, header + 4, lists);
    }
    // what the far kernels gave back (chunks that open without a match): once more the LDS shape, which keeps them
    if (retry_list)
      launch_lds(header + kHeaderRetryCount, retry_list, kHeaderRetryTicket, false);
    return hipSuccess;
  }
  if (plan.forced_far != kClassMix)
    launch_far(plan.forced_far, nullptr, nullptr);
  else
    launch_lds(nullptr, nullptr, kClassMix, false);
  return hipSuccess;
}

hipError_t lz4_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes,
    const size_t* out_caps, size_t batch, uint8_t* const* out_ptrs,
    size_t* actual_bytes, hipcompStatus_t* statuses, bool write_out,
    hipStream_t stream, void* temp, size_t temp_bytes)
{
  // More chunks than the chip holds waves: a persistent grid that draws its chunks from a ticket counter
  // (lz4_decode.hiph), else a wave per chunk by position.  The counter is ONE word of the caller's temp buffer,
  // zeroed on the stream -- a different word for every call of the process (a running call number, modulo the
  // buffer's words: 6 per chunk by the size contract, i.e. at least 49 152 where tickets are used at all), so
  // that calls in flight at once on several streams may share one temp buffer, as they may with the reference,
  // which never touches it (src/lowlevel/LZ4CompressionKernels.hip:224-249; tests/test_lz4_gpu.py:
  // test_concurrent_decompress_calls_share_one_temp_buffer).
  static std::atomic<uint32_t> calls{0};
  const Lz4DecompressPlan plan = lz4_plan_decompress(
      batch, (uint32_t)num_cus_of_current_device(), (unsigned)(reinterpret_cast<uintptr_t>(temp) & 15u),
      temp ? temp_bytes : 0);
  uint32_t* ticket = nullptr;
  if (plan.ticket_words) {
    ticket = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(temp)
                                         + plan.ticket_offset(calls.fetch_add(1, std::memory_order_relaxed)));
    // (a kernel, not hipMemsetAsync: with the memset, a graph captured from compress + decompress replayed
    // with wrong bytes in round 4 -- tests/test_graph_capture_gpu.py; with the kernel it does not)
    lz4_zero_words_kernel<<<dim3(1), dim3(1), 0, stream>>>(ticket);
    const hipError_t zeroed = hipGetLastError();
    if (zeroed != hipSuccess)
      return zeroed;
  }
  const dim3 grid(plan.grid);
  const dim3 block(kWave * kDecompWavesPerBlock);
  if (write_out)
    lz4_decompress_kernel<true><<<grid, block, 0, stream>>>(
        comp_ptrs, comp_bytes, out_caps, batch, out_ptrs, actual_bytes, statuses, ticket);
  else
    lz4_decompress_kernel<false><<<grid, block, 0, stream>>>(
        comp_ptrs, comp_bytes, nullptr, batch, nullptr, actual_bytes, nullptr, ticket);
  return hipSuccess;
}

} // namespace hcamd
