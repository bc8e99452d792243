// gather_kernels.hip -- the kernels of a read of many byte ranges of a container in one call (gather_launch.hpp;
// the arithmetic they share with the host: gather_plan.hpp).
//
// The plan: one workgroup checks every range and takes the exclusive sum of the lengths (where each range lands in
// out), a kernel sets the bit of every chunk some range touches, and the exclusive popcount sum over the bitmap's
// words numbers the touched chunks -- the RANK of a chunk, which says in which pass and into which scratch slot it
// is decoded, once, however many ranges touch it.  Per pass the list kernel writes the chunk list the batched
// decoders and the checksum kernels take (the stored checksums gathered next to it), and the copy kernels move
// every piece from its slot to its range: a range of up to kGatherSmallBytes by 16 lanes, a longer one by a
// workgroup per piece, both with single bytes up to the first 16-byte boundary of the destination, 16-byte
// aligned stores fed by 16-byte loads wherever they lie (legal on gfx950: wave_utils.hpp), and single bytes behind
// the last whole block -- range_slices_kernel's copy.  Plain vector stores only.
#include "gather_launch.hpp"
#include "hlif_container.hpp"
#include "wave_utils.hpp"

namespace hcamd {

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 1024; // = gather::kRankGroup
constexpr int kScanWaves = kScanBlock / kWave;
constexpr int kGroupLanes = 16; // lanes that copy a small range
static_assert(kScanBlock == (int)gather::kRankGroup, "a group of the rank sum is one workgroup's words");

// the test of range_list_kernel (range_kernels.hip)
__device__ __forceinline__ bool header_ok(const RangeContainer& c, uint64_t decomp_bytes, uint64_t chunk_bytes)
{
  const hlif::CommonHeader* h = reinterpret_cast<const hlif::CommonHeader*>(c.container);
  return h->format == c.format && h->uncomp_chunk_size == chunk_bytes && h->num_chunks == c.num_chunks
         && h->decomp_data_size == decomp_bytes && h->comp_data_offset == c.data_at
         && c.num_chunks == (decomp_bytes + chunk_bytes - 1) / chunk_bytes;
}

// wave64 inclusive scan with the saturating sum (wave_utils.hpp's wave_scan_add_u64 with gather::sat_add; lanes
// shifted in from outside read 0, its identity)
__device__ __forceinline__ uint64_t wave_scan_sat_u64(uint64_t v)
{
#define HC_STEP(CTRL, MASK)                                                      \
  {                                                                              \
    const uint64_t u = (uint64_t)dpp_u32<CTRL, MASK>((uint32_t)v)                \
                       | ((uint64_t)dpp_u32<CTRL, MASK>((uint32_t)(v >> 32)) << 32); \
    v = gather::sat_add(v, u);                                                   \
  }
  HC_STEP(0x111, 0xF)
  HC_STEP(0x112, 0xF)
  HC_STEP(0x114, 0xF)
  HC_STEP(0x118, 0xF)
  HC_STEP(0x142, 0xA)
  HC_STEP(0x143, 0xC)
#undef HC_STEP
  return v;
}

__global__ __launch_bounds__(kBlock) void gather_zero_kernel(uint32_t* bitmap, uint64_t words, GatherHead* head)
{
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t == 0) {
    head->touched = 0;
    head->long_ranges = 0;
    head->long_span = 0;
  }
  for (uint64_t w = t; w < words; w += (uint64_t)gridDim.x * kBlock)
    bitmap[w] = 0;
}

// One workgroup: 1024 ranges a step, the sum carried from step to step.
__global__ __launch_bounds__(kScanBlock) void gather_check_kernel(GatherCall g, RangeContainer c, uint64_t out_bytes,
                                                                  hipcompStatus_t* status)
{
  __shared__ uint64_t wave_sums[kScanWaves];
  __shared__ uint32_t bad;
  const int lane = lane_id(), wave = (int)(threadIdx.x / kWave);
  if (threadIdx.x == 0)
    bad = 0;
  __syncthreads();
  uint64_t carry = 0;
  for (uint64_t base = 0; base < g.ranges; base += kScanBlock) {
    const uint64_t r = base + threadIdx.x;
    uint64_t n = 0;
    if (r < g.ranges) {
      n = g.num[r];
      if (!gather::range_valid(g.decomp_bytes, g.first[r], n, g.elem)) {
        bad = 1;
        n = 0;
      }
    }
    const uint64_t incl = wave_scan_sat_u64(n);
    if (lane == kWave - 1)
      wave_sums[wave] = incl;
    __syncthreads();
    uint64_t before = carry, all = carry;
    for (int w = 0; w < kScanWaves; ++w) {
      const uint64_t s = wave_sums[w];
      if (w < wave)
        before = gather::sat_add(before, s);
      all = gather::sat_add(all, s);
    }
    // (a saturated sum makes incl - n meaningless: the call is refused then and the offsets are not looked at)
    if (r < g.ranges)
      g.offs[r] = gather::sat_add(before, incl - n);
    carry = all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    g.offs[g.ranges] = carry;
    const bool refused = bad != 0 || gather::total_refused(carry, out_bytes);
    const bool hbad = !header_ok(c, g.decomp_bytes, g.chunk_bytes);
    g.head->refused = refused ? 1u : 0u;
    g.head->header_bad = hbad ? 1u : 0u;
    g.head->total_bytes = carry;
    *status = refused ? hipcompErrorInvalidValue : hbad ? hipcompErrorCannotDecompress : hipcompSuccess;
  }
}

// bits [lo, hi] of a word
__device__ __forceinline__ uint32_t bits_from_to(uint32_t lo, uint32_t hi)
{
  return (hi >= 31u ? ~0u : (2u << hi) - 1u) & ~((1u << lo) - 1u);
}

// the bits of `mask` in word w: thousands of ranges may hit one chunk, so the word is looked at with a plain load
// first (a stale 0 costs one atomic more; bits are only ever set)
__device__ __forceinline__ void mark(uint32_t* bitmap, uint64_t w, uint32_t mask)
{
  if ((bitmap[w] & mask) != mask)
    atomicOr(&bitmap[w], mask);
}

// A lane per range.  A range inside one word of the bitmap sets its bits itself; one that reaches further is
// spread over the lanes of its wave, a word per lane.
__global__ __launch_bounds__(kBlock) void gather_mark_kernel(GatherCall g, size_t* device_out_offsets)
{
  if (g.head->refused | g.head->header_bad)
    return;
  const int lane = lane_id();
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (device_out_offsets) {
    if (r < g.ranges)
      device_out_offsets[r] = (size_t)g.offs[r];
    if (r == 0)
      device_out_offsets[g.ranges] = (size_t)g.offs[g.ranges];
  }
  uint64_t c0 = 0, c1 = 0;
  bool live = false, is_long = false;
  if (r < g.ranges) {
    const uint64_t n = g.num[r];
    if (n) {
      const gather::Interval iv = gather::range_chunks(g.chunk_bytes, g.first[r], n);
      c0 = iv.c0;
      c1 = iv.c1;
      live = true;
      is_long = n > kGatherSmallBytes;
    }
  }
  // the long ranges: one atomic per wave takes their places in the list
  const uint64_t longs = wave_ballot(is_long);
  if (longs) {
    const int leader = __builtin_ctzll(longs);
    uint32_t at = 0;
    if (lane == leader)
      at = atomicAdd(&g.head->long_ranges, (uint32_t)__builtin_popcountll(longs));
    at = (uint32_t)__shfl((int)at, leader);
    if (is_long) {
      g.long_list[at + (uint32_t)__builtin_popcountll(longs & low_lanes_mask(lane))] = (uint32_t)r;
      const uint64_t span = c1 - c0 + 1;
      atomicMax(&g.head->long_span, (uint32_t)(span > 0xFFFFFFFFull ? 0xFFFFFFFFull : span));
    }
  }
  const bool one_word = (c0 >> 5) == (c1 >> 5);
  if (live && one_word)
    mark(g.bitmap, c0 >> 5, bits_from_to((uint32_t)(c0 & 31), (uint32_t)(c1 & 31)));
  uint64_t many = wave_ballot(live && !one_word);
  while (many) {
    const int src = __builtin_ctzll(many);
    many &= many - 1;
    const uint64_t a = (uint64_t)__shfl((unsigned long long)c0, src), b = (uint64_t)__shfl((unsigned long long)c1, src);
    for (uint64_t w = (a >> 5) + (uint64_t)lane; w <= (b >> 5); w += kWave)
      mark(g.bitmap, w, bits_from_to(w == (a >> 5) ? (uint32_t)(a & 31) : 0u, w == (b >> 5) ? (uint32_t)(b & 31) : 31u));
  }
}

// set bits in front of each word inside its group of 1024 words; group_rank[g] = the group's total
__global__ __launch_bounds__(kScanBlock) void gather_rank_words_kernel(GatherCall g)
{
  __shared__ uint32_t wave_sums[kScanWaves];
  const int lane = lane_id(), wave = (int)(threadIdx.x / kWave);
  const uint64_t w = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  const uint32_t n = w < g.words ? (uint32_t)__builtin_popcount(g.bitmap[w]) : 0u;
  const uint32_t incl = wave_scan_add_u32(n);
  if (lane == kWave - 1)
    wave_sums[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int k = 0; k < kScanWaves; ++k) {
    const uint32_t s = wave_sums[k];
    if (k < wave)
      before += s;
    all += s;
  }
  if (w < g.words)
    g.word_rank[w] = before + incl - n;
  if (threadIdx.x == 0)
    g.group_rank[blockIdx.x] = all;
}

// group totals to the set bits in front of each group, in place; the grand total is the number of touched chunks
__global__ __launch_bounds__(kScanBlock) void gather_rank_groups_kernel(GatherCall g, uint64_t groups)
{
  __shared__ uint32_t wave_sums[kScanWaves];
  const int lane = lane_id(), wave = (int)(threadIdx.x / kWave);
  uint32_t carry = 0;
  for (uint64_t base = 0; base < groups; base += kScanBlock) {
    const uint64_t i = base + threadIdx.x;
    const uint32_t n = i < groups ? g.group_rank[i] : 0u;
    const uint32_t incl = wave_scan_add_u32(n);
    if (lane == kWave - 1)
      wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = carry, all = carry;
    for (int k = 0; k < kScanWaves; ++k) {
      const uint32_t s = wave_sums[k];
      if (k < wave)
        before += s;
      all += s;
    }
    if (i < groups)
      g.group_rank[i] = before + incl - n;
    carry = all;
    __syncthreads();
  }
  if (threadIdx.x == 0)
    g.head->touched = carry;
}

__device__ __forceinline__ uint64_t rank_of(const GatherCall& g, uint64_t c)
{
  const uint64_t w = c >> 5;
  return (uint64_t)g.word_rank[w] + g.group_rank[w / gather::kRankGroup]
         + (uint32_t)__builtin_popcount(g.bitmap[w] & gather::below((uint32_t)(c & 31)));
}

// A lane per word of the bitmap: every set bit whose rank lies in the pass.
__global__ __launch_bounds__(kBlock) void gather_list_kernel(GatherCall g, RangeContainer c, uint64_t sizes_at,
                                                             uint64_t comp_sums_at, uint64_t decomp_sums_at, uint64_t S,
                                                             uint64_t pass, uint32_t count, RangeSlots slots, GatherLists l,
                                                             hipcompStatus_t* status)
{
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= g.words)
    return;
  uint32_t word = g.bitmap[w];
  if (!word)
    return;
  uint64_t rank = (uint64_t)g.word_rank[w] + g.group_rank[w / gather::kRankGroup];
  const uint64_t lo = pass * S, hi = lo + count;
  if (rank >= hi || rank + (uint32_t)__builtin_popcount(word) <= lo)
    return;
  const bool ok = header_ok(c, g.decomp_bytes, g.chunk_bytes);
  for (; word; word &= word - 1, ++rank) {
    if (rank < lo || rank >= hi)
      continue;
    const uint64_t k = rank - lo; // < count <= S: inside the lists and the slots
    if (!ok) {
      l.comp_ptrs[k] = c.container;
      l.comp_sizes[k] = 1;
      l.out_ptrs[k] = slots.base;
      l.caps[k] = 0;
      l.comp_sums[k] = 0;
      l.decomp_sums[k] = 0;
      *status = hipcompErrorCannotDecompress;
      continue;
    }
    // (a set bit is a chunk below ceil(decomp_bytes / chunk_bytes) = num_chunks: inside the container's arrays)
    const uint64_t chunk = w * 32 + (uint32_t)__builtin_ctz(word);
    l.comp_ptrs[k] = c.container + c.data_at + reinterpret_cast<const uint64_t*>(c.container + c.offsets_at)[chunk];
    l.comp_sizes[k] = (size_t) reinterpret_cast<const uint64_t*>(c.container + sizes_at)[chunk];
    l.out_ptrs[k] = slots.base + k * slots.stride;
    l.caps[k] = (size_t)gather::chunk_cap(g.decomp_bytes, g.chunk_bytes, chunk);
    l.comp_sums[k] = reinterpret_cast<const uint32_t*>(c.container + comp_sums_at)[chunk];
    l.decomp_sums[k] = reinterpret_cast<const uint32_t*>(c.container + decomp_sums_at)[chunk];
  }
}

__device__ __forceinline__ bool slot_failed(const GatherLists& l, uint64_t k)
{
  return l.statuses[k] != hipcompSuccess || l.caps[k] == 0 || l.actual[k] != l.caps[k];
}

// n bytes dst <- src by `threads` lanes of which this is lane t (range_slices_kernel's copy)
__device__ __forceinline__ void copy_piece(gptr dst, cgptr src, uint64_t n, uint64_t t, uint64_t threads)
{
  uint64_t head = (16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  if (head > n)
    head = n;
  if (t < head)
    dst[t] = src[t];
  dst += head;
  src += head;
  n -= head;
  const uint64_t nvec = n >> 4;
  uint64_t k = t;
  // 4 x 16 B in flight per lane
  for (; k + 3 * threads < nvec; k += 4 * threads) {
    const u32x4 a = load_u128_any(src + 16 * k);
    const u32x4 b = load_u128_any(src + 16 * (k + threads));
    const u32x4 c = load_u128_any(src + 16 * (k + 2 * threads));
    const u32x4 d = load_u128_any(src + 16 * (k + 3 * threads));
    *reinterpret_cast<HC_GLOBAL u32x4*>(dst + 16 * k) = a;
    *reinterpret_cast<HC_GLOBAL u32x4*>(dst + 16 * (k + threads)) = b;
    *reinterpret_cast<HC_GLOBAL u32x4*>(dst + 16 * (k + 2 * threads)) = c;
    *reinterpret_cast<HC_GLOBAL u32x4*>(dst + 16 * (k + 3 * threads)) = d;
  }
  for (; k < nvec; k += threads)
    *reinterpret_cast<HC_GLOBAL u32x4*>(dst + 16 * k) = load_u128_any(src + 16 * k);
  const uint64_t tail = n & 15u;
  if (t < tail)
    dst[(nvec << 4) + t] = src[(nvec << 4) + t];
}

// the pieces of range r that the pass holds, by `threads` lanes (this one: t; stripe `part` of `parts` of the chunks)
__device__ __forceinline__ void copy_range(const GatherCall& g, uint64_t r, uint64_t first, uint64_t n, uint8_t* out,
                                           uint64_t S, uint64_t pass, uint32_t count, const RangeSlots& slots,
                                           const GatherLists& l, uint64_t t, uint64_t threads, uint32_t part, uint32_t parts)
{
  const gather::Interval iv = gather::range_chunks(g.chunk_bytes, first, n);
  const uint64_t rank0 = rank_of(g, iv.c0);
  const gather::InPass in = gather::range_in_pass(rank0, iv.c0, iv.c1, S, pass);
  const uint64_t at = g.offs[r];
  for (uint64_t c = in.lo + part; c < in.hi; c += parts) {
    const uint64_t k = gather::rank_in_range(rank0, iv.c0, c) - pass * S;
    if (k >= count) // (not reached: the ranks of a pass are below its count)
      return;
    if (slot_failed(l, k))
      continue; // the chunk failed: out keeps what it had there
    const gather::Piece p = gather::range_piece(g.decomp_bytes, g.chunk_bytes, first, n, c);
    copy_piece(to_global(out + at + p.dst_at), to_global(slots.base + k * slots.stride + p.src_at), p.bytes, t, threads);
  }
}

// 16 lanes per range of up to kGatherSmallBytes
__global__ __launch_bounds__(kBlock) void gather_small_kernel(GatherCall g, uint8_t* out, uint64_t S, uint64_t pass,
                                                              uint32_t count, RangeSlots slots, GatherLists l)
{
  const uint64_t r = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kGroupLanes;
  if (r >= g.ranges)
    return;
  const uint64_t n = g.num[r];
  if (n == 0 || n > kGatherSmallBytes)
    return;
  copy_range(g, r, g.first[r], n, out, S, pass, count, slots, l, threadIdx.x % kGroupLanes, kGroupLanes, 0, 1);
}

// long range blockIdx.x of the list, stripe blockIdx.y of its chunks, part blockIdx.z of every piece
__global__ __launch_bounds__(kBlock) void gather_long_kernel(GatherCall g, uint8_t* out, uint64_t S, uint64_t pass,
                                                             uint32_t count, RangeSlots slots, GatherLists l)
{
  const uint64_t r = g.long_list[blockIdx.x];
  copy_range(g, r, g.first[r], g.num[r], out, S, pass, count, slots, l, (uint64_t)blockIdx.z * kBlock + threadIdx.x,
             (uint64_t)gridDim.z * kBlock, blockIdx.y, gridDim.y);
}

} // namespace

hipError_t gather_launch_plan(const GatherCall& g, const RangeContainer& c, uint64_t out_bytes, size_t* device_out_offsets,
                              hipcompStatus_t* status, hipStream_t stream)
{
  uint64_t zero_blocks = (g.words + kBlock - 1) / kBlock;
  zero_blocks = zero_blocks < 1 ? 1 : zero_blocks > 4096 ? 4096 : zero_blocks;
  gather_zero_kernel<<<(uint32_t)zero_blocks, kBlock, 0, stream>>>(g.bitmap, g.words, g.head);
  gather_check_kernel<<<1, kScanBlock, 0, stream>>>(g, c, out_bytes, status);
  gather_mark_kernel<<<(uint32_t)((g.ranges + kBlock - 1) / kBlock), kBlock, 0, stream>>>(g, device_out_offsets);
  const uint64_t groups = (g.words + gather::kRankGroup - 1) / gather::kRankGroup;
  gather_rank_words_kernel<<<(uint32_t)groups, kScanBlock, 0, stream>>>(g);
  gather_rank_groups_kernel<<<1, kScanBlock, 0, stream>>>(g, groups);
  return hipGetLastError();
}

hipError_t gather_launch_list(const GatherCall& g, const RangeContainer& c, uint64_t sizes_at, uint64_t comp_sums_at,
                              uint64_t decomp_sums_at, uint64_t S, uint64_t pass, uint32_t count, const RangeSlots& slots,
                              const GatherLists& l, hipcompStatus_t* status, hipStream_t stream)
{
  if (count == 0)
    return hipSuccess;
  gather_list_kernel<<<(uint32_t)((g.words + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
      g, c, sizes_at, comp_sums_at, decomp_sums_at, S, pass, count, slots, l, status);
  return hipGetLastError();
}

hipError_t gather_launch_copy(const GatherCall& g, uint8_t* out, uint64_t S, uint64_t pass, uint32_t count,
                              uint32_t long_ranges, uint32_t long_span, const RangeSlots& slots, const GatherLists& l,
                              hipStream_t stream)
{
  if (count == 0)
    return hipSuccess;
  if (long_ranges < g.ranges)
    gather_small_kernel<<<(uint32_t)((g.ranges * kGroupLanes + kBlock - 1) / kBlock), kBlock, 0, stream>>>(g, out, S, pass,
                                                                                                          count, slots, l);
  if (long_ranges) {
    // a stripe per chunk a long range may have in the pass (up to 64: the rest in turns), and as
    // range_launch_slices a workgroup per 32 KiB of a piece, up to 128
    uint32_t stripes = long_span < count ? long_span : count;
    stripes = stripes < 1 ? 1 : stripes > 64 ? 64 : stripes;
    uint64_t parts = g.chunk_bytes / 32768;
    parts = parts < 1 ? 1 : parts > 128 ? 128 : parts;
    gather_long_kernel<<<dim3(long_ranges, stripes, (uint32_t)parts), kBlock, 0, stream>>>(g, out, S, pass, count, slots, l);
  }
  return hipGetLastError();
}

} // namespace hcamd
