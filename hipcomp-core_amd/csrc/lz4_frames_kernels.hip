// lz4_frames_kernels.hip -- the kernels of a read of a batch of LZ4 frames in one call (lz4_frames_launch.hpp; the
// arithmetic: lz4_frames_plan.hpp; the passes they make up: hlif.hip).
//
// An item is what decompress_frame reads as `frames`, or an Arrow IPC buffer: eight bytes of length in front of it.
// Every item has a walk's state of its own in the scratch space.  One lane of a wave per item follows the item's
// block chain -- first to count its data blocks; a scan of the counts numbers the blocks through the batch; then,
// pass by pass, to list the item's blocks of the pass at their place in the pass's lists, with the item's number
// beside each.  From there a pass is a single frame read's pass (lz4_frame_device.hiph has the bodies): sizes from a
// parse, places from a scan that starts anew with every item, the batched decoder for the compressed blocks of
// independent-block frames, a copy for the stored ones (and the items that are stored whole), one wave per linked
// frame, the checksums.  What any of them finds goes to the verdict word of the entry's item and to no other.
// Every store is a vector store.
#include "lz4_frames_launch.hpp"

#include "device_facts.hpp"
#include "lz4_frame_device.hiph"

namespace hcamd {
namespace lz4fb {

using namespace lz4f;

namespace {

struct ItemOf
{
  Item* items;
  const uint32_t* col;
  __device__ __forceinline__ uint32_t* verdict(uint32_t e) const { return &items[col[e]].st.verdict; }
  __device__ __forceinline__ uint8_t* out(uint32_t e) const { return items[col[e]].out; }
  __device__ __forceinline__ uint64_t carried_start(uint32_t e) const { return items[col[e]].st.frame_out_start; }
};

__device__ __forceinline__ uint64_t read64(const uint8_t* p) { return (uint64_t)read32(p) | ((uint64_t)read32(p + 4) << 32); }

__device__ __forceinline__ ReadState fresh_state()
{
  ReadState z = {};
  z.all_declared = 1;
  z.cur_content = kNoContentSize;
  return z;
}

__device__ __forceinline__ ReadLists lists_from(const ReadLists& l, uint64_t at)
{
  ReadLists r;
  r.comp_ptrs = l.comp_ptrs + at;
  r.comp_bytes = l.comp_bytes + at;
  r.batch_bytes = l.batch_bytes + at;
  r.sizes = l.sizes + at;
  r.out_ptrs = l.out_ptrs + at;
  r.caps = l.caps + at;
  r.batch_caps = l.batch_caps + at;
  r.actual = l.actual + at;
  r.aux = l.aux + at;
  r.flags = l.flags + at;
  r.head = l.head + at;
  r.statuses = l.statuses + at;
  return r;
}

// The three walks: wave w of the grid takes items w, w + waves, ...; lane 0 of it does the work and the other
// lanes wait at the end of the loop body (read_walk leaves its loop from many places: no second lane goes in).
#define HC_ITEMS_OF_WAVE(it, num_items)                                                                                \
  for (uint64_t it = (uint64_t)blockIdx.x * kWavesPerBlock + uniform((uint32_t)(threadIdx.x >> 6)); it < (num_items);   \
       it += (uint64_t)gridDim.x * kWavesPerBlock)

__global__ __launch_bounds__(kBlock) void begin_kernel(Batch b, Item* items, bool sizes_only)
{
  const bool worker = lane_id() == 0;
  HC_ITEMS_OF_WAVE(it, b.items)
  {
    if (!worker)
      continue;
    const uint8_t* const p = b.item_ptrs[it];
    const uint64_t bytes = b.item_bytes[it];
    const uint64_t capacity = b.out_ptrs ? (uint64_t)b.out_capacities[it] : ~uint64_t(0);
    const uint64_t word = b.prefix == kArrowLength && bytes >= 8 ? read64(p) : 0;
    const PrefixPlan plan = prefix_plan(b.prefix, bytes, word, capacity);
    Item z = {};
    z.st = fresh_state();
    z.kind = plan.kind;
    z.in = p + plan.payload_at;
    z.n = bytes - plan.payload_at;
    z.out = b.out_ptrs ? b.out_ptrs[it] : nullptr;
    z.expected = plan.expected;
    z.room = plan.expected != kNoExpectedSize ? plan.expected : capacity;
    if (plan.kind == kRaw) {
      z.blocks = z.n ? 1 : 0;
      z.st.pos = z.n;
      z.st.done = 1;
    }
    if (plan.kind == kEmpty) // (nothing to walk: the end of the input is where it stands)
      z.st.done = 1;
    items[it] = z;
    if (plan.kind != kFrames)
      continue;
    read_walk(z.in, z.n, &items[it].st, ReadLists(), false, 0, false, false);
    const ReadState h = items[it].st;
    if (h.reason != kOk)
      continue; // (no blocks, the reason stands)
    if (sizes_only && h.all_declared) {
      items[it].kind = kDeclared;
      continue;
    }
    items[it].blocks = (uint32_t)h.blocks; // (the walk refuses more than 2^32 - 1)
    items[it].st = fresh_state();
  }
}

__global__ __launch_bounds__(kScanBlock) void scan_items_kernel(Item* items, uint64_t num_items, Totals* totals)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  __shared__ unsigned long long largest;
  if (threadIdx.x == 0)
    largest = 0;
  __syncthreads();
  uint64_t base = 0, mine = 0;
  for (uint64_t tile = 0; tile < num_items; tile += kScanBlock) {
    const uint64_t i = tile + threadIdx.x;
    uint64_t v = 0;
    if (i < num_items) {
      v = items[i].blocks;
      const uint64_t n = items[i].n, most = items[i].kind == kRaw ? n : (n < (4u << 20) ? n : (4u << 20));
      if (v && most > mine)
        mine = most;
    }
    uint64_t total;
    const uint64_t excl = block_scan(v, lds, total);
    if (i < num_items)
      items[i].first = base + excl;
    base += total;
  }
  atomicMax(&largest, (unsigned long long)mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    totals->blocks = base;
    totals->largest = largest;
  }
}

__global__ __launch_bounds__(kBlock) void list_kernel(Item* items, uint64_t num_items, ReadLists l, uint32_t* item_col,
                                                      uint64_t P, uint64_t k, bool verify)
{
  const bool worker = lane_id() == 0;
  HC_ITEMS_OF_WAVE(it, num_items)
  {
    if (!worker)
      continue;
    const Slice s = item_slice(items[it].first, items[it].blocks, P, k);
    if (s.count == 0)
      continue;
    const ReadLists mine = lists_from(l, s.at);
    if (items[it].kind == kRaw) { // (one block, this one)
      mine.comp_ptrs[0] = items[it].in;
      mine.comp_bytes[0] = (size_t)items[it].n;
      mine.batch_bytes[0] = 0;
      mine.flags[0] = kStored | kLast | kRawItem;
      mine.head[0] = 0;
      mine.aux[0] = kNoContentSize;
    } else {
      read_walk(items[it].in, items[it].n, &items[it].st, mine, true, (uint32_t)s.count, false, verify);
    }
    // (the walk numbers a frame's first entry from the front of the lists it was given)
    for (uint64_t j = 0; j < s.count; ++j) {
      item_col[s.at + j] = (uint32_t)it;
      if (mine.head[j] >= 0)
        mine.head[j] += (int32_t)s.at;
    }
  }
}

__global__ void linked_sizes_kernel(ReadLists l, uint32_t count)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count)
    return;
  const uint32_t flags = l.flags[i];
  if (!(flags & kLinked) || (flags & kStored))
    return;
  l.sizes[i] = linked_block_size(l.comp_ptrs[i], (uint32_t)l.comp_bytes[i]);
}

// One workgroup.  First the sum of the sizes before every entry of the pass, kept in caps[]; then every entry's place
// in its item's buffer: that sum less the one at the item's first entry of the pass, from the item's cursor on; then
// caps[] itself, the declared sizes of the frames that end here, and the cursors.
__global__ __launch_bounds__(kScanBlock) void place_kernel(Item* items, ReadLists l, const uint32_t* item_col, uint32_t count,
                                                          uint64_t pass_first)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  uint64_t base = 0;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t e = tile + threadIdx.x;
    uint64_t size = 0;
    if (e < count) {
      const uint32_t flags = l.flags[e];
      size = (flags & kStored) ? l.comp_bytes[e] : (flags & kLinked) ? l.sizes[e] : l.actual[e];
      if (!(flags & kRawItem) && size > block_max_of_code((flags >> 8) & 7u)) {
        atomicOr(&items[item_col[e]].st.verdict, kVerdictCannotDecompress);
        size = 0;
      }
    }
    uint64_t total;
    const uint64_t before = base + block_scan(size, lds, total);
    if (e < count) {
      l.caps[e] = (size_t)before;
      l.sizes[e] = (size_t)size;
    }
    base += total;
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < count; e += kScanBlock) {
    const uint32_t it = item_col[e], flags = l.flags[e];
    const uint64_t first = items[it].first, room = items[it].room;
    const uint32_t front = first > pass_first ? (uint32_t)(first - pass_first) : 0; // the item's first entry here
    const uint64_t off = items[it].st.out_cursor + ((uint64_t)l.caps[e] - (uint64_t)l.caps[front]);
    uint64_t size = l.sizes[e];
    if (e + 1 == count || item_col[e + 1] != it)
      items[it].next_cursor = off + size;
    if (off > room || size > room - off) { // no room: the block gets none
      atomicOr(&items[it].st.verdict, kVerdictCannotDecompress);
      size = 0;
    }
    l.sizes[e] = (size_t)size;
    l.out_ptrs[e] = items[it].out + (off < room ? off : room);
    l.batch_caps[e] = (flags & (kStored | kLinked)) ? 0 : (size_t)size;
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < count; e += kScanBlock) {
    const uint32_t it = item_col[e];
    l.caps[e] = l.sizes[e];
    if (e + 1 == count || item_col[e + 1] != it)
      items[it].st.out_cursor = items[it].next_cursor;
    // a frame that ends in this pass and declares its size: from its first byte to its last block's end
    if (!(l.flags[e] & kLast) || l.aux[e] == kNoContentSize)
      continue;
    const uint8_t* const out = items[it].out;
    const int32_t head = l.head[e];
    const uint64_t start = head >= 0 ? (uint64_t)(l.out_ptrs[head] - out) : items[it].st.frame_out_start;
    const uint64_t end = (uint64_t)(l.out_ptrs[e] - out) + l.sizes[e];
    if (end - start != l.aux[e])
      atomicOr(&items[it].st.verdict, kVerdictCannotDecompress);
  }
}

__global__ void batched_verdict_kernel(Item* items, ReadLists l, const uint32_t* item_col, uint32_t count)
{
  batched_verdict_of_thread(l, count, ItemOf{items, item_col});
}

__global__ __launch_bounds__(kBlock) void stored_kernel(ReadLists l, uint32_t count)
{
  const uint32_t i = blockIdx.x;
  if (i >= count || !(l.flags[i] & kStored))
    return;
  strided_copy(to_global(l.out_ptrs[i]), to_global(l.comp_ptrs[i]), l.caps[i], (uint64_t)blockIdx.y * kBlock + threadIdx.x,
               (uint64_t)gridDim.y * kBlock);
}

// one wave per linked frame of the pass, whatever item it belongs to; frame_start of a frame that began in an
// earlier pass comes from its item's state
__global__ __launch_bounds__(kBlock) void linked_kernel(Item* items, ReadLists l, const uint32_t* item_col, uint32_t count)
{
  linked_frame_of_wave(l, count, ItemOf{items, item_col});
}

__global__ void block_sums_kernel(Item* items, ReadLists l, const uint32_t* item_col, uint32_t count)
{
  block_sum_of_quad(l, count, ItemOf{items, item_col});
}

__global__ __launch_bounds__(kBlock) void content_sums_kernel(Item* items, ReadLists l, const uint32_t* item_col, uint32_t count)
{
  content_sum_of_wave(l, count, ItemOf{items, item_col});
}

__global__ void pass_end_kernel(Item* items, ReadLists l, const uint32_t* item_col, uint32_t count)
{
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= count)
    return;
  const uint32_t it = item_col[e];
  if (e + 1 != count && item_col[e + 1] == it)
    return;
  const int32_t head = l.head[e];
  if (head >= 0)
    items[it].st.frame_out_start = (uint64_t)(l.out_ptrs[head] - items[it].out);
}

// statuses == nullptr: the size query
__global__ __launch_bounds__(kBlock) void finish_kernel(Item* items, uint64_t num_items, bool verify, bool require, size_t* sizes,
                                                        hipcompStatus_t* statuses)
{
  const bool worker = lane_id() == 0;
  HC_ITEMS_OF_WAVE(it, num_items)
  {
    if (!worker)
      continue;
    const uint32_t kind = items[it].kind;
    if (!statuses) {
      const ReadState st = items[it].st;
      sizes[it] = (size_t)(kind == kDeclared ? st.declared_sum : kind == kRefused || st.reason != kOk ? 0 : st.out_cursor);
      continue;
    }
    // what lies behind the last block (trailers are read with their block; skippable and empty frames here)
    if (kind == kFrames)
      read_walk(items[it].in, items[it].n, &items[it].st, ReadLists(), true, 0, true, verify);
    const ReadState st = items[it].st;
    const uint64_t expected = items[it].expected;
    hipcompStatus_t status = hipcompSuccess;
    if (kind == kRefused)
      status = hipcompErrorCannotDecompress;
    else if (st.verdict & kVerdictBadChecksum)
      status = hipcompErrorBadChecksum;
    else if (st.reason != kOk)
      status = (hipcompStatus_t)status_of(st.reason);
    else if ((st.verdict & kVerdictCannotDecompress) || !st.done || (expected != kNoExpectedSize && st.out_cursor != expected))
      status = hipcompErrorCannotDecompress;
    else if (require && (st.bare_frames != 0 || kind == kRaw))
      status = hipcompErrorCannotVerifyChecksums;
    statuses[it] = status;
    sizes[it] = status == hipcompSuccess || status == hipcompErrorCannotVerifyChecksums ? (size_t)st.out_cursor : 0;
  }
}

__global__ void prefix_sizes_kernel(Batch b, size_t* sizes)
{
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= b.items)
    return;
  const uint64_t bytes = b.item_bytes[i];
  sizes[i] = (size_t)prefix_size(bytes, bytes >= 8 ? read64(b.item_ptrs[i]) : 0);
}

// workgroups of a walk over num_items items: a wave each, no more than the device holds at once
uint32_t walk_groups(const void* kernel, uint64_t num_items)
{
  const uint64_t want = (num_items + kWavesPerBlock - 1) / kWavesPerBlock;
  const int per_cu = resident_per_cu(kernel, kBlock, 0);
  const uint64_t most = (uint64_t)num_cus_of_current_device() * (uint64_t)(per_cu > 0 ? per_cu : 1);
  return (uint32_t)(want < most ? want : most);
}

} // namespace

hipError_t launch_begin(const Batch& b, Item* items, bool sizes_only, hipStream_t stream)
{
  begin_kernel<<<walk_groups((const void*)begin_kernel, b.items), kBlock, 0, stream>>>(b, items, sizes_only);
  return hipGetLastError();
}

hipError_t launch_scan_items(Item* items, uint64_t num_items, Totals* totals, hipStream_t stream)
{
  scan_items_kernel<<<1, kScanBlock, 0, stream>>>(items, num_items, totals);
  return hipGetLastError();
}

hipError_t launch_list(Item* items, uint64_t num_items, const ReadLists& l, uint32_t* item_col, uint64_t P, uint64_t k, bool verify,
                       hipStream_t stream)
{
  list_kernel<<<walk_groups((const void*)list_kernel, num_items), kBlock, 0, stream>>>(items, num_items, l, item_col, P, k, verify);
  return hipGetLastError();
}

hipError_t launch_linked_sizes(const ReadLists& l, uint32_t count, hipStream_t stream)
{
  linked_sizes_kernel<<<groups(count), kBlock, 0, stream>>>(l, count);
  return hipGetLastError();
}

hipError_t launch_place(Item* items, const ReadLists& l, const uint32_t* item_col, uint32_t count, uint64_t pass_first,
                        hipStream_t stream)
{
  place_kernel<<<1, kScanBlock, 0, stream>>>(items, l, item_col, count, pass_first);
  return hipGetLastError();
}

hipError_t launch_batched_verdict(Item* items, const ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream)
{
  batched_verdict_kernel<<<groups(count), kBlock, 0, stream>>>(items, l, item_col, count);
  return hipGetLastError();
}

hipError_t launch_stored(const ReadLists& l, uint32_t count, uint64_t largest_block, hipStream_t stream)
{
  stored_kernel<<<dim3(count, parts_of(largest_block)), kBlock, 0, stream>>>(l, count);
  return hipGetLastError();
}

hipError_t launch_linked(Item* items, const ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream)
{
  linked_kernel<<<groups((uint64_t)count * kWave), kBlock, 0, stream>>>(items, l, item_col, count);
  return hipGetLastError();
}

hipError_t launch_block_sums(Item* items, const ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream)
{
  block_sums_kernel<<<groups(4ull * count), kBlock, 0, stream>>>(items, l, item_col, count);
  return hipGetLastError();
}

hipError_t launch_content_sums(Item* items, const ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream)
{
  content_sums_kernel<<<groups((uint64_t)count * kWave), kBlock, 0, stream>>>(items, l, item_col, count);
  return hipGetLastError();
}

hipError_t launch_pass_end(Item* items, const ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream)
{
  pass_end_kernel<<<groups(count), kBlock, 0, stream>>>(items, l, item_col, count);
  return hipGetLastError();
}

hipError_t launch_finish(Item* items, uint64_t num_items, bool verify, bool require_checksums, size_t* sizes,
                         hipcompStatus_t* statuses, hipStream_t stream)
{
  finish_kernel<<<walk_groups((const void*)finish_kernel, num_items), kBlock, 0, stream>>>(items, num_items, verify,
                                                                                           require_checksums, sizes, statuses);
  return hipGetLastError();
}

hipError_t launch_prefix_sizes(const Batch& b, size_t* sizes, hipStream_t stream)
{
  prefix_sizes_kernel<<<groups(b.items), kBlock, 0, stream>>>(b, sizes);
  return hipGetLastError();
}

} // namespace lz4fb
} // namespace hcamd
