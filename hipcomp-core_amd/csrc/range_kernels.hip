// range_kernels.hip -- the kernels of a ranged read of a container (range_launch.hpp; the plan they share with
// the host: range_plan.hpp).
//
// The list kernel is the ranged counterpart of hlif.hip's slab_streams_kernel: the same test of the container's
// header, and a chunk list that holds only the range's chunks.  Interior chunks are decoded straight into the
// caller's buffer; an edge chunk is decoded whole into a scratch slot, and the slice kernel moves the wanted span
// from there.  Source (slot + src_at) and destination (out + dst_at) of a span lie at any two byte alignments:
// the copy stores 16 bytes per lane at 16-byte aligned addresses and loads 16 bytes per lane wherever they lie
// (legal on gfx950: wave_utils.hpp), with single bytes in front of the first and behind the last aligned block.
#include "hlif_container.hpp"
#include "range_launch.hpp"
#include "wave_utils.hpp"

namespace hcamd {

namespace {

constexpr int kListBlock = 256;
constexpr int kCopyBlock = 256;

__global__ void range_list_kernel(RangeContainer c, range::Plan plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                                  RangeSlots slots, const uint8_t** comp_ptrs, uint8_t** out_ptrs, size_t* caps,
                                  hipcompStatus_t* status)
{
  const uint32_t i = blockIdx.x * kListBlock + threadIdx.x;
  if (i >= count)
    return;
  const hlif::CommonHeader* h = reinterpret_cast<const hlif::CommonHeader*>(c.container);
  const bool header_ok = h->format == c.format && h->uncomp_chunk_size == plan.chunk_bytes
                         && h->num_chunks == c.num_chunks && h->decomp_data_size == plan.decomp_bytes
                         && h->comp_data_offset == c.data_at
                         && c.num_chunks == (plan.decomp_bytes + plan.chunk_bytes - 1) / plan.chunk_bytes;
  if (!header_ok) {
    comp_ptrs[i] = c.container;
    out_ptrs[i] = slots.base;
    caps[i] = 0;
    *status = hipcompErrorCannotDecompress;
    return;
  }
  // (the plan's chunks lie below ceil(decomp_bytes / chunk_bytes) = num_chunks: inside the offsets array)
  const uint64_t chunk = pass_first + i;
  const uint64_t off = reinterpret_cast<const uint64_t*>(c.container + c.offsets_at)[chunk];
  const range::Span s = range::range_span(plan, chunk, pass_first);
  comp_ptrs[i] = c.container + c.data_at + off;
  out_ptrs[i] = s.edge ? slots.base + (uint64_t)s.slot * slots.stride : out + s.dst_at;
  caps[i] = (size_t)s.cap;
}

// Edge candidate blockIdx.x of the pass (every chunk where the plan says all_edge, else the pass's first and last
// chunk), part blockIdx.y of gridDim.y: a workgroup-strided loop over the span's aligned 16-byte blocks.
__global__ __launch_bounds__(kCopyBlock) void range_slices_kernel(
    range::Plan plan, uint64_t pass_first, uint32_t count, uint8_t* out, RangeSlots slots,
    const hipcompStatus_t* statuses, const size_t* actual, const size_t* caps)
{
  uint32_t i = blockIdx.x;
  if (!plan.all_edge) {
    if (blockIdx.x == 1 && count == 1)
      return;
    i = blockIdx.x == 0 ? 0 : count - 1;
  }
  const range::Span s = range::range_span(plan, pass_first + i, pass_first);
  if (!s.edge)
    return;
  if (statuses[i] != hipcompSuccess || caps[i] == 0 || actual[i] != caps[i])
    return; // the chunk failed: out keeps what it had there
  cgptr src = to_global(slots.base + (uint64_t)s.slot * slots.stride + s.src_at);
  gptr dst = to_global(out + s.dst_at);
  uint64_t n = s.bytes;
  const uint64_t t = (uint64_t)blockIdx.y * kCopyBlock + threadIdx.x, threads = (uint64_t)gridDim.y * kCopyBlock;
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

__global__ void range_finish_kernel(const bool* comp_flag, const bool* decomp_flag, const CrcState* st, bool require,
                                    hipcompStatus_t* status)
{
  const uint32_t flags = st->flags;
  if (flags & kCrcNoHeader)
    return; // the header check failed: its status stands, nothing was compared
  if (flags & kCrcBad)
    *status = hipcompErrorBadChecksum;
  else if (require && !(*comp_flag && *decomp_flag) && *status == hipcompSuccess)
    *status = hipcompErrorCannotVerifyChecksums;
}

} // namespace

hipError_t range_launch_list(const RangeContainer& c, const range::Plan& plan, uint64_t pass_first, uint32_t count,
                             uint8_t* out, const RangeSlots& slots, const uint8_t** comp_ptrs, uint8_t** out_ptrs,
                             size_t* caps, hipcompStatus_t* status, hipStream_t stream)
{
  if (count == 0)
    return hipSuccess;
  range_list_kernel<<<(count + kListBlock - 1) / kListBlock, kListBlock, 0, stream>>>(
      c, plan, pass_first, count, out, slots, comp_ptrs, out_ptrs, caps, status);
  return hipGetLastError();
}

hipError_t range_launch_slices(const range::Plan& plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                               const RangeSlots& slots, const hipcompStatus_t* statuses, const size_t* actual,
                               const size_t* caps, hipStream_t stream)
{
  if (count == 0)
    return hipSuccess;
  // a span is at most a chunk: one workgroup per 32 KiB of it, up to 128
  uint64_t parts = plan.chunk_bytes / 32768;
  parts = parts < 1 ? 1 : parts > 128 ? 128 : parts;
  const dim3 grid(plan.all_edge ? count : range::kTwoEdges, (uint32_t)parts);
  range_slices_kernel<<<grid, kCopyBlock, 0, stream>>>(plan, pass_first, count, out, slots, statuses, actual, caps);
  return hipGetLastError();
}

hipError_t range_launch_finish(const bool* comp_flag, const bool* decomp_flag, const CrcState* st, bool require,
                               hipcompStatus_t* status, hipStream_t stream)
{
  range_finish_kernel<<<1, 1, 0, stream>>>(comp_flag, decomp_flag, st, require, status);
  return hipGetLastError();
}

} // namespace hcamd
