// checksum_kernels.hip -- the CRC-32 passes of the high-level managers (checksum_launch.hpp says how hlif.hip
// drives them; crc32_math.hpp holds the definition and the algebra).
//
// The chunk CRC kernel: one wave per chunk, grid-stride over the list.  A chunk's 16-byte aligned middle is
// cut into 64 contiguous per-lane segments of whole 16-byte blocks; lane 0 also takes the bytes in front of
// the first aligned block, the lane with the last block the bytes behind it.  Each lane folds its segment in
// with 16-byte global loads and slice-by-16 tables in LDS (16 lookups per 16 bytes), and the segments are
// joined by crc32_shift: the chunk's CRC is the XOR over the lanes of shift(segment CRC, bytes behind the
// segment).  With 64 KiB chunks the segments are 1 KiB and those shifts are multiples of 1 KiB: popcount(63 -
// lane) multiplications mod P per lane.  The CRC joins the pass word shifted by the bytes of the pass behind
// the chunk; those shifts are gathered one per lane and done 64 at a time, so that a wave does not wait on
// one lane's square-and-multiply after every chunk.
#include "checksum_launch.hpp"
#include "crc32_math.hpp"
#include "device_facts.hpp"
#include "wave_utils.hpp"

namespace hcamd {

namespace {

__device__ const crc32::Tables kCrcTables = crc32::make_tables();
__device__ const crc32::ShiftTable kCrcShift = crc32::make_shift_table();

constexpr int kCrcBlock = 256;  // 4 waves: 4 chunks at a time per workgroup
constexpr int kScanBlock = 1024;

struct LdsTables
{
  crc32::Tables s;
  uint32_t x2n[crc32::kShiftBits];
};

__device__ __forceinline__ size_t chunk_len(const CrcChunks& c, uint32_t i, bool& skip)
{
  size_t len = 0;
  skip = false;
  if (c.caps) {
    const size_t cap = c.caps[i];
    if (cap == 0) {
      skip = true;
      return 0;
    }
    len = c.lens[i];
    if (c.clamp_to_caps && cap < len)
      len = cap;
    return len;
  }
  return c.lens[i];
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
  for (int d = 1; d < kWave; d <<= 1)
    v ^= (uint32_t)__shfl_xor((int)v, d, kWave);
  return v;
}

// the CRC of p[0, n), all 64 lanes of the wave, the result in every lane
__device__ __forceinline__ uint32_t wave_crc(const LdsTables& L, const uint8_t* p, uint64_t n, int lane)
{
  const uintptr_t start = reinterpret_cast<uintptr_t>(p), end = start + n;
  const uintptr_t a = (start + 15) & ~uintptr_t(15), b = end & ~uintptr_t(15);
  const uint64_t nblk = b > a ? (b - a) / 16 : 0;
  uint64_t s = 0, e = 0;               // this lane's 16-byte blocks [s, e) from a
  const uint8_t* head = p;             // bytes in front of the blocks (lane 0) ...
  uint64_t head_n = 0, tail_n = 0;     // ... and behind them (the lane with the last block)
  uint64_t seg_end = 0;                // where this lane's segment ends (bytes from p)
  if (nblk == 0) {
    if (lane == 0) {
      head_n = n;
      seg_end = n;
    }
  } else {
    const uint64_t per = (nblk + kWave - 1) / kWave;
    s = (uint64_t)lane * per;
    e = s + per;
    s = s < nblk ? s : nblk;
    e = e < nblk ? e : nblk;
    if (lane == 0)
      head_n = a - start;
    if (e == nblk && s < e)
      tail_n = end - b;
    seg_end = (a - start) + e * 16 + tail_n;
  }
  uint32_t reg = 0xFFFFFFFFu;
  reg = crc32::crc32_update_bytes(L.s.t[0], reg, head, head_n);
  const HC_GLOBAL u32x4* q = reinterpret_cast<const HC_GLOBAL u32x4*>(a);
  uint64_t j = s;
  for (; j + 4 <= e; j += 4) {
    const u32x4 v0 = q[j], v1 = q[j + 1], v2 = q[j + 2], v3 = q[j + 3];
    reg = crc32::crc32_update_16(L.s, reg, v0.x, v0.y, v0.z, v0.w);
    reg = crc32::crc32_update_16(L.s, reg, v1.x, v1.y, v1.z, v1.w);
    reg = crc32::crc32_update_16(L.s, reg, v2.x, v2.y, v2.z, v2.w);
    reg = crc32::crc32_update_16(L.s, reg, v3.x, v3.y, v3.z, v3.w);
  }
  for (; j < e; ++j) {
    const u32x4 v = q[j];
    reg = crc32::crc32_update_16(L.s, reg, v.x, v.y, v.z, v.w);
  }
  reg = crc32::crc32_update_bytes(L.s.t[0], reg, reinterpret_cast<const uint8_t*>(b), tail_n);
  const bool any = head_n + tail_n + (e - s) * 16 != 0;
  const uint32_t crc = any ? crc32::crc32_shift(L.x2n, ~reg, n - seg_end) : 0u;
  return wave_xor(crc);
}

__device__ __forceinline__ void fill_tables(LdsTables& L)
{
  const u32x4* src = reinterpret_cast<const u32x4*>(&kCrcTables);
  u32x4* dst = reinterpret_cast<u32x4*>(&L.s);
  for (uint32_t k = threadIdx.x; k < sizeof(crc32::Tables) / 16; k += blockDim.x)
    dst[k] = src[k];
  if (threadIdx.x < crc32::kShiftBits)
    L.x2n[threadIdx.x] = kCrcShift.x2n[threadIdx.x];
  __syncthreads();
}

__global__ __launch_bounds__(kCrcBlock) void crc_chunks_kernel(CrcChunks c, CrcTarget t)
{
  __shared__ LdsTables L;
  fill_tables(L);
  if (t.present && !*t.present)
    return;
  const int lane = lane_id();
  const uint64_t pass_bytes = t.pass_bytes_dev ? *t.pass_bytes_dev : t.pass_bytes;
  uint32_t acc = 0, pend_crc = 0;
  uint64_t pend_shift = 0;
  int pending = 0;
  const uint32_t waves = gridDim.x * (kCrcBlock / kWave);
  for (uint32_t i = blockIdx.x * (kCrcBlock / kWave) + threadIdx.x / kWave; i < c.count; i += waves) {
    bool skip;
    const size_t len = chunk_len(c, i, skip);
    if (skip) {
      if (lane == 0)
        atomicOr(t.flags, kCrcNoHeader);
      continue;
    }
    const uint8_t* p = c.ptrs ? c.ptrs[i] : c.base + c.offsets[i];
    const uint32_t crc = wave_crc(L, p, len, lane);
    if (lane == 0) {
      if (t.values)
        t.values[i] = crc;
      else if (t.stored[i] != crc)
        atomicOr(t.flags, kCrcBad);
    }
    const uint64_t before = t.before ? t.before[i] + t.before[c.count + i / kScanBlock] : (uint64_t)i * t.stride;
    if (lane == pending) {
      pend_crc = crc;
      pend_shift = pass_bytes - before - len;
    }
    if (++pending == kWave) {
      acc ^= crc32::crc32_shift(L.x2n, pend_crc, pend_shift);
      pend_crc = 0;
      pend_shift = 0;
      pending = 0;
    }
  }
  if (pending)
    acc ^= crc32::crc32_shift(L.x2n, pend_crc, pend_shift);
  acc = wave_xor(acc);
  if (lane == 0 && acc)
    atomicXor(t.pass_word, acc);
}

// the bytes in front of each chunk inside its group of 1024, and each group's total
__global__ __launch_bounds__(kScanBlock) void crc_scan_groups_kernel(CrcChunks c, uint64_t* work)
{
  __shared__ uint64_t wave_sums[kScanBlock / kWave];
  const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
  bool skip;
  const uint64_t len = i < c.count ? chunk_len(c, i, skip) : 0;
  const uint64_t incl = wave_scan_add_u64(len);
  const int w = threadIdx.x / kWave;
  if (lane_id() == kWave - 1)
    wave_sums[w] = incl;
  __syncthreads();
  uint64_t in_front = 0;
  for (int k = 0; k < w; ++k)
    in_front += wave_sums[k];
  if (i < c.count)
    work[i] = in_front + incl - len;
  if (threadIdx.x == kScanBlock - 1)
    work[c.count + blockIdx.x] = in_front + incl; // the group's total, made the bytes in front of it below
}

// the group totals into the bytes in front of each group (exclusive scan in place), and the pass's total
__global__ __launch_bounds__(kScanBlock) void crc_scan_totals_kernel(uint32_t groups, uint64_t* totals, CrcState* st)
{
  __shared__ uint64_t wave_sums[kScanBlock / kWave];
  const uint32_t g = threadIdx.x;
  const uint64_t v = g < groups ? totals[g] : 0;
  const uint64_t incl = wave_scan_add_u64(v);
  const int w = threadIdx.x / kWave;
  if (lane_id() == kWave - 1)
    wave_sums[w] = incl;
  __syncthreads();
  uint64_t in_front = 0;
  for (int k = 0; k < w; ++k)
    in_front += wave_sums[k];
  if (g < groups)
    totals[g] = in_front + incl - v;
  if (g == kScanBlock - 1)
    st->comp_pass_bytes = in_front + incl;
}

__global__ void crc_reset_kernel(CrcState* st)
{
  st->comp_acc = st->decomp_acc = st->comp_pass = st->decomp_pass = 0;
  st->comp_pass_bytes = 0;
  st->flags = 0;
}

__global__ void crc_fold_kernel(CrcState* st, uint64_t decomp_pass_bytes)
{
  st->comp_acc = crc32::crc32_shift(kCrcShift.x2n, st->comp_acc, st->comp_pass_bytes) ^ st->comp_pass;
  st->decomp_acc = crc32::crc32_shift(kCrcShift.x2n, st->decomp_acc, decomp_pass_bytes) ^ st->decomp_pass;
  st->comp_pass = st->decomp_pass = 0;
  st->comp_pass_bytes = 0;
}

__global__ void crc_finish_compress_kernel(
    uint32_t* full_comp, uint32_t* full_decomp, bool* comp_flag, bool* decomp_flag, const CrcState* st)
{
  *full_comp = st->comp_acc;
  *full_decomp = st->decomp_acc;
  *comp_flag = true;
  *decomp_flag = true;
}

__global__ void crc_finish_decompress_kernel(const uint32_t* full_comp, const uint32_t* full_decomp, const bool* comp_flag,
                                             const bool* decomp_flag, const CrcState* st, bool require,
                                             hipcompStatus_t* status)
{
  const uint32_t flags = st->flags;
  if (flags & kCrcNoHeader)
    return; // the header check failed: its status stands, nothing was compared
  const bool has_comp = *comp_flag, has_decomp = *decomp_flag;
  const bool bad = (flags & kCrcBad) || (has_comp && *full_comp != st->comp_acc)
                   || (has_decomp && *full_decomp != st->decomp_acc);
  if (bad)
    *status = hipcompErrorBadChecksum;
  else if (require && !(has_comp && has_decomp) && *status == hipcompSuccess)
    *status = hipcompErrorCannotVerifyChecksums;
}

} // namespace

hipError_t crc_launch_reset(CrcState* st, hipStream_t stream)
{
  crc_reset_kernel<<<1, 1, 0, stream>>>(st);
  return hipGetLastError();
}

hipError_t crc_launch_scan(const CrcChunks& c, uint64_t* work, CrcState* st, hipStream_t stream)
{
  const uint32_t groups = (c.count + kScanBlock - 1) / kScanBlock;
  if (groups > kScanBlock)
    return hipErrorInvalidValue;
  if (groups)
    crc_scan_groups_kernel<<<groups, kScanBlock, 0, stream>>>(c, work);
  crc_scan_totals_kernel<<<1, kScanBlock, 0, stream>>>(groups, work + c.count, st);
  return hipGetLastError();
}

hipError_t crc_launch_chunks(const CrcChunks& c, const CrcTarget& t, hipStream_t stream)
{
  if (c.count == 0)
    return hipSuccess;
  const uint32_t per_group = kCrcBlock / kWave;
  const uint32_t want = (c.count + per_group - 1) / per_group;
  // enough workgroups to fill every CU (the LDS tables hold 9 per CU), few enough that each copies its tables
  // for many chunks
  const uint32_t cap = (uint32_t)num_cus_of_current_device() * 8;
  crc_chunks_kernel<<<want < cap ? want : cap, kCrcBlock, 0, stream>>>(c, t);
  return hipGetLastError();
}

hipError_t crc_launch_fold(CrcState* st, uint64_t decomp_pass_bytes, hipStream_t stream)
{
  crc_fold_kernel<<<1, 1, 0, stream>>>(st, decomp_pass_bytes);
  return hipGetLastError();
}

hipError_t crc_launch_finish_compress(uint32_t* full_comp, uint32_t* full_decomp, bool* comp_flag, bool* decomp_flag,
                                      const CrcState* st, hipStream_t stream)
{
  crc_finish_compress_kernel<<<1, 1, 0, stream>>>(full_comp, full_decomp, comp_flag, decomp_flag, st);
  return hipGetLastError();
}

hipError_t crc_launch_finish_decompress(const uint32_t* full_comp, const uint32_t* full_decomp, const bool* comp_flag,
                                        const bool* decomp_flag, const CrcState* st, bool require,
                                        hipcompStatus_t* status, hipStream_t stream)
{
  crc_finish_decompress_kernel<<<1, 1, 0, stream>>>(full_comp, full_decomp, comp_flag, decomp_flag, st, require, status);
  return hipGetLastError();
}

} // namespace hcamd
