// gzip_kernels.hip -- the device side of include/hipcomp/gzip.h: what stands around a raw Deflate stream in a gzip
// member, a zlib stream or a BGZF block.  The Deflate work itself is the two Deflate libraries'; these kernels run
// in front of and behind their launches (gzip_batch.cpp has the order).
//
//   gzip_parse_kernel    decode, first: one thread per member runs gzipframe::parse_member -- the function
//                        tests/test_gzip_frame_cpu.py proves -- and leaves the payload span and the trailer's words
//   gzip_verify_kernel   decode, last: one wave per member takes the checksum of the decoded bytes, compares it
//                        (and ISIZE) with the trailer and writes the caller's actual / statuses
//   gzip_list_kernel     encode, first: where the raw encoder writes, the wrapper's header length behind out_i
//   gzip_frame_kernel    encode, last: one wave per chunk takes the checksum of the input chunk and writes header
//                        and trailer around the stream
//
// The checksum of a chunk (wave_crc32, wave_adler32) is the hot part.  The chunk's 16-byte aligned middle is cut
// into 64 contiguous per-lane segments of whole 16-byte blocks, read with 16-byte loads, the next four already in
// flight while four are folded in; lane 0 also takes the bytes in front of the first aligned block and the lane
// that holds the last block the bytes behind it, one at a time, so that nothing outside [p, p + n) is read.  CRC-32
// folds 16 bytes with the slice-by-16 tables in LDS and joins the segments by crc32_shift (crc32_math.hpp);
// Adler-32 needs no table and joins them by the sums of adler32_math.hpp.
#include "gzip_launch.hpp"

#include "adler32_math.hpp"
#include "crc32_math.hpp"
#include "gzip_frame.hpp"
#include "wave_utils.hpp"

namespace hcamd {

namespace {

__device__ const crc32::Tables kGzipCrcTables = crc32::make_tables();
__device__ const crc32::ShiftTable kGzipCrcShift = crc32::make_shift_table();

constexpr int kBlock = 256;                  // 4 waves: 4 chunks at a time per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
// Workgroups of a checksum launch, at most: 8 on each of an MI355X's 256 CUs (the 16.3 KiB of tables admit 9), so
// that each copies its tables once for many chunks; a larger batch is walked grid-stride.
constexpr size_t kMaxBlocks = 256 * 8;

struct CrcLds
{
  crc32::Tables s;
  uint32_t x2n[crc32::kShiftBits];
};

// What one lane reads of a chunk: `head_n` single bytes at `head`, the 16-byte blocks [s, e) of `blocks`, `tail_n`
// single bytes at `tail`, all contiguous, with `after` bytes of the chunk behind them.
struct Segment
{
  cgptr head, tail;
  const HC_GLOBAL u32x4* blocks;
  uint64_t s, e, after;
  uint32_t head_n, tail_n;
};

__device__ __forceinline__ Segment segment_of(const uint8_t* p, uint64_t n, int lane)
{
  const uintptr_t start = reinterpret_cast<uintptr_t>(p), end = start + n;
  const uintptr_t first = (start + 15) & ~uintptr_t(15), last = end & ~uintptr_t(15);
  Segment g;
  g.head = reinterpret_cast<cgptr>(start);
  g.tail = reinterpret_cast<cgptr>(last);
  g.blocks = reinterpret_cast<const HC_GLOBAL u32x4*>(first);
  g.s = g.e = 0;
  g.head_n = g.tail_n = 0;
  g.after = 0;
  if (last <= first) {   // no whole aligned block (n < 31): lane 0 reads the chunk byte by byte
    if (lane == 0)
      g.head_n = (uint32_t)n;
    return g;
  }
  const uint64_t nblk = (last - first) / 16;
  const uint64_t per = (nblk + kWave - 1) / kWave;
  const uint64_t s = (uint64_t)lane * per, e = s + per;
  g.s = s < nblk ? s : nblk;
  g.e = e < nblk ? e : nblk;
  if (lane == 0)
    g.head_n = (uint32_t)(first - start);
  if (g.e == nblk && g.s < g.e)
    g.tail_n = (uint32_t)(end - last);
  g.after = n - ((first - start) + g.e * 16 + g.tail_n);
  return g;
}

// fold(v) for every 16-byte block of the segment in order; the loads of the next four blocks are issued before
// the current four are folded
template <typename Fold>
__device__ __forceinline__ void for_each_block(const Segment& g, Fold fold)
{
  uint64_t j = g.s;
  if (j + 4 <= g.e) {
    u32x4 v0 = g.blocks[j], v1 = g.blocks[j + 1], v2 = g.blocks[j + 2], v3 = g.blocks[j + 3];
    j += 4;
    for (;;) {
      const bool more = j + 4 <= g.e;
      u32x4 n0 = v0, n1 = v1, n2 = v2, n3 = v3;
      if (more) {
        n0 = g.blocks[j];
        n1 = g.blocks[j + 1];
        n2 = g.blocks[j + 2];
        n3 = g.blocks[j + 3];
      }
      fold(v0);
      fold(v1);
      fold(v2);
      fold(v3);
      if (!more)
        break;
      v0 = n0;
      v1 = n1;
      v2 = n2;
      v3 = n3;
      j += 4;
    }
  }
  for (; j < g.e; ++j)
    fold(g.blocks[j]);
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
  for (int d = 1; d < kWave; d <<= 1)
    v ^= (uint32_t)__shfl_xor((int)v, d, kWave);
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
  for (int d = 1; d < kWave; d <<= 1)
    v += (uint32_t)__shfl_xor((int)v, d, kWave);
  return v;
}

// CRC-32 of p[0, n), all 64 lanes of the wave, the result in every lane.  A lane without bytes has the CRC 0,
// which any shift leaves 0.
__device__ __forceinline__ uint32_t wave_crc32(const CrcLds& L, const uint8_t* p, uint64_t n, int lane)
{
  const Segment g = segment_of(p, n, lane);
  uint32_t reg = 0xFFFFFFFFu;
  for (uint32_t k = 0; k < g.head_n; ++k)
    reg = (reg >> 8) ^ L.s.t[0][(reg ^ g.head[k]) & 0xFFu];
  for_each_block(g, [&](u32x4 v) { reg = crc32::crc32_update_16(L.s, reg, v.x, v.y, v.z, v.w); });
  for (uint32_t k = 0; k < g.tail_n; ++k)
    reg = (reg >> 8) ^ L.s.t[0][(reg ^ g.tail[k]) & 0xFFu];
  return wave_xor(crc32::crc32_shift(L.x2n, ~reg, g.after));
}

// Adler-32 of p[0, n), all 64 lanes of the wave, the result in every lane.  Between two reductions a lane takes
// at most 15 single bytes and 344 blocks (5519 bytes, below adler32::kNmax), whichever end of its segment they
// are at.
__device__ __forceinline__ uint32_t wave_adler32(const uint8_t* p, uint64_t n, int lane)
{
  constexpr uint32_t kBlocksBetween = adler32::kBlocksPerReduce - 3;
  static_assert(kBlocksBetween * 16 + 15 <= adler32::kNmax, "a lane's bytes between two reductions");
  const Segment g = segment_of(p, n, lane);
  uint32_t a = 0, b = 0, left = kBlocksBetween;
  for (uint32_t k = 0; k < g.head_n; ++k) {
    a += g.head[k];
    b += a;
  }
  for_each_block(g, [&](u32x4 v) {
    adler32::update_16(a, b, v.x, v.y, v.z, v.w);
    if (--left == 0) {
      a %= adler32::kMod;
      b %= adler32::kMod;
      left = kBlocksBetween;
    }
  });
  for (uint32_t k = 0; k < g.tail_n; ++k) {
    a += g.tail[k];
    b += a;
  }
  const adler32::Piece piece{a % adler32::kMod, b % adler32::kMod};
  // 64 terms below 65521 each: the sums stay far below 2^32
  return adler32::finish(wave_sum(piece.a), wave_sum(adler32::b_share(piece, g.after)), n);
}

__device__ __forceinline__ void fill_tables(CrcLds& L)
{
  const u32x4* src = reinterpret_cast<const u32x4*>(&kGzipCrcTables);
  u32x4* dst = reinterpret_cast<u32x4*>(&L.s);
  for (uint32_t k = threadIdx.x; k < sizeof(crc32::Tables) / 16; k += kBlock)
    dst[k] = src[k];
  if (threadIdx.x < crc32::kShiftBits)
    L.x2n[threadIdx.x] = kGzipCrcShift.x2n[threadIdx.x];
  __syncthreads();
}

// the wrapper's checksum of p[0, n): kAdler is the same for the whole launch
template <bool kAdler>
__device__ __forceinline__ uint32_t wave_checksum(const CrcLds& L, const uint8_t* p, uint64_t n, int lane)
{
  if constexpr (kAdler)
    return wave_adler32(p, n, lane);
  else
    return wave_crc32(L, p, n, lane);
}

__global__ __launch_bounds__(kBlock) void gzip_parse_kernel(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t batch, int wrapper, GzipDecodeTemp t)
{
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= batch)
    return;
  const uint8_t* p = comp_ptrs[i];
  const gzipframe::Member m = gzipframe::parse_member(p, comp_bytes[i], wrapper);
  t.payload_ptrs[i] = m.ok ? p + m.payload_at : p;
  t.payload_bytes[i] = m.ok ? m.payload_bytes : 0;
  t.checks[i] = m.check;
  t.isizes[i] = m.isize;
  t.header_ok[i] = m.ok ? 1u : 0u;
}

template <bool kAdler>
__global__ __launch_bounds__(kBlock) void gzip_verify_kernel(
    const uint8_t* const* out_ptrs, size_t batch, GzipDecodeTemp t, size_t* actual, hipcompStatus_t* statuses)
{
  __shared__ CrcLds L;
  if constexpr (!kAdler)
    fill_tables(L);
  const int lane = lane_id();
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t i = (size_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; i < batch; i += waves) {
    hipcompStatus_t st = hipcompErrorCannotDecompress;
    size_t act = 0;
    const bool decoded = uniform(t.header_ok[i]) != 0 && uniform((uint32_t)t.raw_statuses[i]) == (uint32_t)hipcompSuccess;
    if (decoded) {
      const uint64_t len = uniform((uint64_t)t.raw_actual[i]);
      const uint32_t sum = wave_checksum<kAdler>(L, uniform_ptr(out_ptrs[i]), len, lane);
      const bool same = sum == t.checks[i] && (kAdler || t.isizes[i] == (uint32_t)len);
      st = same ? hipcompSuccess : hipcompErrorBadChecksum;
      act = same ? (size_t)len : 0;
    }
    if (lane == 0) {
      if (actual)
        actual[i] = act;
      if (statuses)
        statuses[i] = st;
    }
  }
}

__global__ __launch_bounds__(kBlock) void gzip_list_kernel(
    uint8_t* const* out_ptrs, size_t batch, uint32_t header_len, uint8_t** payload_ptrs)
{
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < batch)
    payload_ptrs[i] = out_ptrs[i] + header_len;
}

template <bool kAdler>
__global__ __launch_bounds__(kBlock) void gzip_frame_kernel(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t batch, int wrapper, uint8_t* const* out_ptrs,
    size_t* out_bytes)
{
  __shared__ CrcLds L;
  if constexpr (!kAdler)
    fill_tables(L);
  const int lane = lane_id();
  const uint32_t header_len = gzipframe::header_bytes(wrapper), trailer_len = gzipframe::trailer_bytes(wrapper);
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t i = (size_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; i < batch; i += waves) {
    const uint64_t stream_bytes = uniform((uint64_t)out_bytes[i]);
    if (stream_bytes == 0)   // the encoder left the chunk out (larger than the call's chunk size): no bytes for it
      continue;
    const uint64_t n = uniform((uint64_t)in_bytes[i]);
    const uint32_t sum = wave_checksum<kAdler>(L, uniform_ptr(in_ptrs[i]), n, lane);
    const uint64_t member_bytes = stream_bytes + header_len + trailer_len;
    gptr out = to_global(uniform_ptr(out_ptrs[i]));
    if ((uint32_t)lane < header_len)
      out[lane] = gzipframe::header_byte(wrapper, (uint32_t)lane, (uint32_t)member_bytes);
    if ((uint32_t)lane < trailer_len)
      out[header_len + stream_bytes + lane] = gzipframe::trailer_byte(wrapper, (uint32_t)lane, sum, (uint32_t)n);
    if (lane == 0)
      out_bytes[i] = (size_t)member_bytes;
  }
}

uint32_t thread_blocks(size_t batch) { return (uint32_t)((batch + kBlock - 1) / kBlock); }

uint32_t wave_blocks(size_t batch)
{
  const size_t want = (batch + kWavesPerBlock - 1) / kWavesPerBlock;
  return (uint32_t)(want < kMaxBlocks ? want : kMaxBlocks);
}

} // namespace

void gzip_launch_parse(const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t batch, int wrapper,
                       const GzipDecodeTemp& t, hipStream_t stream)
{
  gzip_parse_kernel<<<thread_blocks(batch), kBlock, 0, stream>>>(comp_ptrs, comp_bytes, batch, wrapper, t);
}

void gzip_launch_verify(const uint8_t* const* out_ptrs, size_t batch, int wrapper, const GzipDecodeTemp& t,
                        size_t* actual, hipcompStatus_t* statuses, hipStream_t stream)
{
  if (wrapper == gzipframe::kZlib)
    gzip_verify_kernel<true><<<wave_blocks(batch), kBlock, 0, stream>>>(out_ptrs, batch, t, actual, statuses);
  else
    gzip_verify_kernel<false><<<wave_blocks(batch), kBlock, 0, stream>>>(out_ptrs, batch, t, actual, statuses);
}

void gzip_launch_list(uint8_t* const* out_ptrs, size_t batch, int wrapper, uint8_t** payload_ptrs, hipStream_t stream)
{
  gzip_list_kernel<<<thread_blocks(batch), kBlock, 0, stream>>>(
      out_ptrs, batch, gzipframe::header_bytes(wrapper), payload_ptrs);
}

void gzip_launch_frame(const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t batch, int wrapper,
                       uint8_t* const* out_ptrs, size_t* out_bytes, hipStream_t stream)
{
  if (wrapper == gzipframe::kZlib)
    gzip_frame_kernel<true><<<wave_blocks(batch), kBlock, 0, stream>>>(in_ptrs, in_bytes, batch, wrapper, out_ptrs, out_bytes);
  else
    gzip_frame_kernel<false><<<wave_blocks(batch), kBlock, 0, stream>>>(in_ptrs, in_bytes, batch, wrapper, out_ptrs, out_bytes);
}

} // namespace hcamd
