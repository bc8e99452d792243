// deflate_kernels.hip -- batched raw-Deflate (RFC 1951) decoder for gfx950, one chunk per wavefront.
//
// Shape:
//   * kWavesPerBlock waves per workgroup, each with its own slice of LDS; the waves share nothing and never
//     meet at a barrier.  Chunks are taken grid-stride, so the grid is bounded whatever the batch.
//   * The bit position is wave-uniform: the bit buffer, the stream position and every decoded symbol live in
//     scalar registers (uniform() below), the control flow is the scalar unit's.  The buffer is refilled 32
//     bits at a time from a window of 2 x 256 stream bytes that the lanes hold in registers (one aligned dword
//     per lane and window, read with v_readlane); the second window is loaded while the first is consumed.
//   * Decode tables per wave in LDS (deflate_tables.hpp: fast table + count/sorted walk for the longer codes),
//     built by all 64 lanes: ballots count the code lengths and rank the symbols, the fast table is filled in
//     parallel over its entries.
//   * All data movement is wave-wide: stored blocks and matches are 64-lane copies (an overlapping match
//     reads its source modulo the distance), literals collect in a 64-byte LDS queue that is stored with one
//     byte per lane.
//   * Every path checks its bounds first: bits consumed against the stream's size, bytes produced against the
//     capacity, a match distance against the bytes produced.  A chunk that breaks one ends with
//     hipcompErrorCannotDecompress; nothing is read or written outside the chunk's own two ranges.
#include <hip/hip_runtime.h>

#include "deflate_launch.hpp"
#include "deflate_tables.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace {

using namespace deflate;

constexpr int kWavesPerBlock = 4;
// as many waves as the chip holds (256 CUs x 32): a larger batch is walked grid-stride
constexpr unsigned kMaxBlocks = 256u * 32u / kWavesPerBlock;
constexpr int kQueueBytes = kWave;

struct WaveLds
{
  uint16_t lit_fast[1 << kLitFastBits];
  uint16_t dist_fast[1 << kDistFastBits];
  uint16_t cl_fast[1 << kCodeLenFastBits];
  uint16_t lit_sorted[kFixedLitLen];
  uint16_t dist_sorted[kFixedDist];
  uint16_t cl_sorted[32];
  uint16_t lit_count[16];
  uint16_t dist_count[16];
  uint16_t cl_count[16];
  uint8_t lengths[kFixedLitLen + kFixedDist]; // literal/length lengths, then the distance lengths
  uint8_t cl_lengths[32];
  uint8_t queue[kQueueBytes];
};
static_assert(sizeof(WaveLds) <= 6 * 1024, "the per-wave LDS budget of DESIGN.md section 13");

__device__ __forceinline__ uint32_t mod_below_512(uint32_t i, uint32_t m)
{
  // i mod m for i < 512, 1 <= m: quotient from a float reciprocal (off by at most one at these sizes), one
  // correction either way
  const float r = __builtin_amdgcn_rcpf((float)m);
  const uint32_t q = (uint32_t)((float)i * r);
  int32_t rem = (int32_t)(i - q * m);
  rem = rem < 0 ? rem + (int32_t)m : rem;
  rem = rem >= (int32_t)m ? rem - (int32_t)m : rem;
  return (uint32_t)rem;
}

// ---- the stream: bit buffer over a register window -----------------------------------------------------------
// Positions are in WINDOW SPACE: byte w lies at address `abase + w`, where abase is the chunk's address rounded
// down to 4 and the stream's byte s is w = skew + s.  Bytes outside [skew, skew + len) read as zero and are never
// loaded.
struct BitStream
{
  cgptr abase;
  uint64_t lo, hi;   // the stream's bytes in window space: [lo, hi)
  uint64_t wpos;     // next byte to enter the bit buffer
  uint64_t w0;       // window space position of win0's lane 0 (a multiple of 4)
  uint64_t buf;
  uint32_t cnt;
  uint32_t win0, win1; // per lane

  __device__ __forceinline__ uint32_t load_window(uint64_t base, int lane) const
  {
    const uint64_t p = base + 4u * (uint32_t)lane;
    uint32_t v = 0;
    if (p >= lo && p + 4u <= hi) {
      v = *reinterpret_cast<const HC_GLOBAL uint32_t*>(abase + p);
    } else if (p + 4u > lo && p < hi) { // the dword that holds the stream's first or last bytes: byte by byte
      for (uint32_t b = 0; b < 4u; ++b)
        if (p + b >= lo && p + b < hi)
          v |= (uint32_t)abase[p + b] << (8u * b);
    }
    return v;
  }

  __device__ __forceinline__ void seek(uint64_t w, int lane)
  {
    wpos = w;
    w0 = w & ~(uint64_t)3;
    buf = 0;
    cnt = 0;
    win0 = load_window(w0, lane);
    win1 = load_window(w0 + 256u, lane);
  }

  __device__ __forceinline__ void init(const uint8_t* comp, size_t len, int lane)
  {
    const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(comp);
    abase = to_global(reinterpret_cast<const uint8_t*>(a & ~(uint64_t)3));
    lo = a & 3u;
    hi = lo + len;
    seek(lo, lane);
  }

  // at least 33 bits in the buffer afterwards
  __device__ __forceinline__ void refill(int lane)
  {
    if (cnt <= 32u) {
      uint32_t rel = (uint32_t)(wpos - w0);
      if (rel >= 256u) {
        win0 = win1;
        w0 += 256u;
        win1 = load_window(w0 + 256u, lane);
        rel -= 256u;
      }
      const uint32_t idx = rel >> 2;
      const uint32_t a = read_lane(win0, (int)idx);
      const uint32_t b = idx == 63u ? read_lane(win1, 0) : read_lane(win0, (int)((idx + 1u) & 63u));
      const uint32_t v = (uint32_t)((((uint64_t)b << 32) | a) >> ((rel & 3u) * 8u));
      buf |= (uint64_t)v << cnt;
      cnt += 32u;
      wpos += 4u;
    }
  }

  __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }
  __device__ __forceinline__ void drop(uint32_t n)
  {
    buf >>= n;
    cnt -= n;
  }
  __device__ __forceinline__ uint32_t take(uint32_t n) // n < 32
  {
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  __device__ __forceinline__ uint32_t take32()
  {
    const uint32_t v = (uint32_t)buf;
    drop(32u);
    return v;
  }
  // more bits consumed than the stream has (the buffer then holds zero bits from past its end)
  __device__ __forceinline__ bool overrun() const { return wpos * 8u - cnt > hi * 8u; }
  // window space position of the next unread byte (the buffer holds whole bytes)
  __device__ __forceinline__ uint64_t byte_pos() const { return wpos - (cnt >> 3); }
};

// ---- tables, built by the wave ---------------------------------------------------------------------------------
// lengths[0, n) (LDS) -> count / sorted / fast (LDS) and the verdict of deflate_tables.hpp.
template <int FASTBITS>
__device__ __forceinline__ Verdict build_table_wave(
    const uint8_t* lengths, uint32_t n, Kind kind, uint16_t* count, uint16_t* sorted, uint16_t* fast, int lane)
{
  lds_phase();
  uint32_t cnt[kMaxBits + 1];
#pragma unroll
  for (int l = 0; l <= kMaxBits; ++l)
    cnt[l] = 0;
  for (uint32_t base = 0; base < n; base += kWave) {
    const uint32_t len = base + (uint32_t)lane < n ? (uint32_t)lengths[base + lane] : 0u;
#pragma unroll
    for (int l = 1; l <= kMaxBits; ++l)
      cnt[l] += (uint32_t)__builtin_popcountll(wave_ballot(len == (uint32_t)l));
  }
  const Verdict v = verdict_counts(cnt, kind);
  if (v == kOverSubscribed)
    return v;
  uint32_t offs[kMaxBits + 1];
  offs[1] = 0;
#pragma unroll
  for (int l = 2; l <= kMaxBits; ++l)
    offs[l] = offs[l - 1] + cnt[l - 1];
  const uint64_t below = low_lanes_mask(lane);
  for (uint32_t base = 0; base < n; base += kWave) {
    const uint32_t len = base + (uint32_t)lane < n ? (uint32_t)lengths[base + lane] : 0u;
#pragma unroll
    for (int l = 1; l <= kMaxBits; ++l) {
      const uint64_t m = wave_ballot(len == (uint32_t)l);
      if (len == (uint32_t)l)
        sorted[offs[l] + (uint32_t)__builtin_popcountll(m & below)] = (uint16_t)(base + lane);
      offs[l] += (uint32_t)__builtin_popcountll(m);
    }
  }
  if (lane <= kMaxBits) {
    uint32_t mine = 0;
#pragma unroll
    for (int l = 1; l <= kMaxBits; ++l)
      mine = lane == l ? cnt[l] : mine;
    count[lane] = (uint16_t)mine;
  }
  lds_phase();
  for (uint32_t e = (uint32_t)lane; e < (1u << FASTBITS); e += kWave)
    fast[e] = (uint16_t)canon_decode(cnt, sorted, e, FASTBITS);
  lds_phase();
  return v;
}

template <int FASTBITS>
__device__ __forceinline__ uint32_t decode_symbol(
    const uint16_t* fast, const uint16_t* count, const uint16_t* sorted, uint32_t bits)
{
  uint32_t e = uniform((uint32_t)fast[bits & ((1u << FASTBITS) - 1u)]);
  if (e == 0)
    e = uniform(canon_decode(count, sorted, bits, kMaxBits));
  return e;
}

// ---- one chunk ------------------------------------------------------------------------------------------------
// -> true and the decoded size, or false.  WRITE_OUT = false decodes without an output (the size query).
template <bool WRITE_OUT>
__device__ __forceinline__ bool inflate_chunk(
    const uint8_t* comp, size_t comp_len, uint8_t* out_generic, size_t cap, WaveLds& lds, int lane, size_t& produced)
{
  gptr out = to_global(out_generic);
  BitStream in;
  in.init(comp, comp_len, lane);
  size_t outpos = 0; // bytes stored; the queue holds `qn` more
  uint32_t qn = 0;
  bool fixed_tables = false;

  auto flush = [&]() {
    if (WRITE_OUT) {
      lds_phase();
      if ((uint32_t)lane < qn)
        out[outpos + (uint32_t)lane] = lds.queue[lane];
      lds_phase();
    }
    outpos += qn;
    qn = 0;
  };

  for (;;) {
    in.refill(lane);
    const uint32_t bfinal = in.take(1);
    const uint32_t btype = in.take(2);
    if (in.overrun() || btype == 3u)
      return false;
    if (btype == 0u) {
      // ---- stored: to the byte boundary, LEN, NLEN, then LEN bytes as they are
      in.drop(in.cnt & 7u);
      in.refill(lane);
      const uint32_t word = in.take32();
      if (in.overrun())
        return false;
      const uint32_t n = word & 0xFFFFu;
      if ((n ^ 0xFFFFu) != (word >> 16))
        return false;
      const uint64_t src = in.byte_pos();
      flush();
      if (n > in.hi - src || n > cap - outpos)
        return false;
      if (WRITE_OUT) {
        // 64 bytes per step at any alignment of either side; 16 bytes per lane once the run is long
        if (n >= 1024u) {
          wave_copy(out + outpos, in.abase + src, n, lane);
        } else {
          for (uint32_t i = (uint32_t)lane; i < n; i += kWave)
            out[outpos + i] = in.abase[src + i];
        }
      }
      outpos += n;
      in.seek(src + n, lane);
    } else {
      if (btype == 1u) {
        if (!fixed_tables) {
          for (uint32_t i = (uint32_t)lane; i < (uint32_t)(kFixedLitLen + kFixedDist); i += kWave)
            lds.lengths[i] = (uint8_t)(i < (uint32_t)kFixedLitLen ? fixed_litlen_length(i) : kFixedDistLength);
          build_table_wave<kLitFastBits>(lds.lengths, kFixedLitLen, kLitLen, lds.lit_count, lds.lit_sorted, lds.lit_fast, lane);
          build_table_wave<kDistFastBits>(lds.lengths + kFixedLitLen, kFixedDist, kDist, lds.dist_count, lds.dist_sorted,
                                          lds.dist_fast, lane);
          fixed_tables = true;
        }
      } else {
        // ---- dynamic: HLIT, HDIST, HCLEN, the code-length code, then the two sets of lengths
        fixed_tables = false;
        const uint32_t hlit = in.take(5) + 257u, hdist = in.take(5) + 1u, hclen = in.take(4) + 4u;
        if (in.overrun() || verdict_header(hlit, hdist) != kOk)
          return false;
        if (lane < 32)
          lds.cl_lengths[lane] = 0;
        lds_phase();
        for (uint32_t i = 0; i < hclen; ++i) {
          in.refill(lane);
          lds.cl_lengths[kCodeLenOrder[i]] = (uint8_t)in.take(3);
        }
        if (in.overrun())
          return false;
        if (build_table_wave<kCodeLenFastBits>(lds.cl_lengths, kNumCodeLen, kCodeLen, lds.cl_count, lds.cl_sorted, lds.cl_fast,
                                               lane) != kOk)
          return false;
        const uint32_t total = hlit + hdist;
        uint32_t have = 0, prev = 0;
        while (have < total) {
          in.refill(lane);
          const uint32_t e = decode_symbol<kCodeLenFastBits>(lds.cl_fast, lds.cl_count, lds.cl_sorted, (uint32_t)in.buf);
          if (e == 0)
            return false;
          in.drop(e & 15u);
          const uint32_t sym = e >> 4;
          const uint32_t extra = in.take(code_len_extra_bits(sym));
          uint32_t value = 0, count = 0;
          if (in.overrun() || code_len_run(sym, extra, have, total, prev, value, count) != kOk)
            return false;
          // the run, up to 138 lengths, with all lanes (have + count <= total <= 316)
          for (uint32_t j = (uint32_t)lane; j < count; j += kWave)
            lds.lengths[have + j] = (uint8_t)value;
          have += count;
          prev = value;
        }
        lds_phase();
        if (uniform((uint32_t)lds.lengths[kEndOfBlock]) == 0u)
          return false;
        if (build_table_wave<kLitFastBits>(lds.lengths, hlit, kLitLen, lds.lit_count, lds.lit_sorted, lds.lit_fast, lane) != kOk)
          return false;
        if (build_table_wave<kDistFastBits>(lds.lengths + hlit, hdist, kDist, lds.dist_count, lds.dist_sorted, lds.dist_fast,
                                            lane) != kOk)
          return false;
      }
      // ---- the block's symbols
      for (;;) {
        in.refill(lane);
        const uint32_t e = decode_symbol<kLitFastBits>(lds.lit_fast, lds.lit_count, lds.lit_sorted, (uint32_t)in.buf);
        if (e == 0)
          return false;
        in.drop(e & 15u);
        const uint32_t sym = e >> 4;
        if (sym < 256u) {
          if (in.overrun() || cap - outpos <= qn)
            return false;
          if (WRITE_OUT)
            lds.queue[qn] = (uint8_t)sym; // (every lane the same byte to the same place)
          if (++qn == (uint32_t)kQueueBytes)
            flush();
          continue;
        }
        if (sym == (uint32_t)kEndOfBlock) {
          if (in.overrun())
            return false;
          break;
        }
        if (sym >= (uint32_t)kMaxLitLen)
          return false; // 286, 287: coded in the fixed block, never legal
        const uint32_t li = sym - 257u;
        const uint32_t mlen = length_base(li) + in.take(length_extra(li));
        in.refill(lane);
        const uint32_t de = decode_symbol<kDistFastBits>(lds.dist_fast, lds.dist_count, lds.dist_sorted, (uint32_t)in.buf);
        if (de == 0)
          return false;
        in.drop(de & 15u);
        const uint32_t dsym = de >> 4;
        if (dsym >= (uint32_t)kMaxDist)
          return false; // 30, 31
        const uint32_t dist = dist_base(dsym) + in.take(dist_extra(dsym));
        if (in.overrun())
          return false;
        flush();
        if (dist > outpos || mlen > cap - outpos)
          return false;
        if (WRITE_OUT) {
          gptr dst = out + outpos;
          cgptr src = static_cast<cgptr>(out) + (outpos - dist);
          if (dist >= mlen) {
            for (uint32_t i = (uint32_t)lane; i < mlen; i += kWave)
              dst[i] = src[i];
          } else {
            // the match runs into its own output: its source repeats with period `dist`, all of it bytes that
            // were stored before the match began
            for (uint32_t i = (uint32_t)lane; i < mlen; i += kWave)
              dst[i] = src[mod_below_512(i, dist)];
          }
        }
        outpos += mlen;
      }
    }
    if (bfinal)
      break;
  }
  flush();
  produced = outpos;
  return true;
}

template <bool WRITE_OUT>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void deflate_decompress_kernel(
    const uint8_t* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes,
    const size_t* __restrict__ out_caps, const size_t batch, uint8_t* const* __restrict__ out_ptrs,
    size_t* __restrict__ actual_bytes, hipcompStatus_t* __restrict__ statuses)
{
  __shared__ WaveLds lds_all[kWavesPerBlock];
  const int lane = lane_id();
  const uint32_t wave = uniform((uint32_t)(threadIdx.x >> 6));
  WaveLds& lds = lds_all[wave];
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t chunk = (size_t)blockIdx.x * kWavesPerBlock + wave; chunk < batch; chunk += waves) {
    const uint8_t* comp = uniform_ptr(comp_ptrs[chunk]);
    const size_t comp_len = (size_t)uniform((uint64_t)comp_bytes[chunk]);
    uint8_t* out = WRITE_OUT ? uniform_ptr(out_ptrs[chunk]) : nullptr;
    const size_t cap = WRITE_OUT ? (size_t)uniform((uint64_t)out_caps[chunk]) : ~(size_t)0;
    size_t produced = 0;
    const bool ok = inflate_chunk<WRITE_OUT>(comp, comp_len, out, cap, lds, lane, produced);
    if (lane == 0) {
      if (actual_bytes != nullptr)
        actual_bytes[chunk] = ok ? produced : 0;
      if (statuses != nullptr)
        statuses[chunk] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
    }
  }
}

unsigned grid_for(size_t batch)
{
  const size_t blocks = (batch + kWavesPerBlock - 1) / kWavesPerBlock;
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

} // namespace

void deflate_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps, size_t batch,
    uint8_t* const* out_ptrs, size_t* actual_bytes, hipcompStatus_t* statuses, hipStream_t stream)
{
  deflate_decompress_kernel<true><<<dim3(grid_for(batch)), dim3(kWave * kWavesPerBlock), 0, stream>>>(
      comp_ptrs, comp_bytes, out_caps, batch, out_ptrs, actual_bytes, statuses);
}

void deflate_launch_get_sizes(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t* out_sizes, size_t batch, hipStream_t stream)
{
  deflate_decompress_kernel<false><<<dim3(grid_for(batch)), dim3(kWave * kWavesPerBlock), 0, stream>>>(
      comp_ptrs, comp_bytes, nullptr, batch, nullptr, out_sizes, nullptr);
}

} // namespace hcamd
