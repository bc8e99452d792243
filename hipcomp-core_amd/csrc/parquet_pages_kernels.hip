// parquet_pages_kernels.hip -- the kernels of a read of the pages of a batch of Parquet column chunks in one call
// (parquet_pages_launch.hpp; the arithmetic and the page rules: parquet_pages_plan.hpp).
//
// An item is a column chunk: a chain of pages, each a Thrift compact-protocol header of unknown length and a body.
// One wavefront per item follows the chain (walk_pages of the plan, the very code the host tests run): first to
// count the item's listed pages and what they decode to; a scan of the counts numbers the pages through the batch;
// then, pass by pass, to list the item's pages of the pass -- a row of its page table each, and an entry of the
// pass's lists: the compressed part for the batched decoder, the stored part for the copy, the body for the CRC.
//
// The walk is wave-uniform: all 64 lanes run the parser on the same state.  The header bytes come through a register
// window: 64 bytes of the chunk in one coalesced load, lane l keeping byte l, every byte the parser asks for read from
// the window's lane with a uniform index (v_readlane), the window loaded anew where the parser leaves it.  So a page
// costs about one dependent global load, not one per Thrift byte; binaries and bodies are stepped over by arithmetic.
// Only lane 0 stores.  Every store is a vector store.
#include "parquet_pages_launch.hpp"

#include "byte_window.hpp"
#include "checksum_launch.hpp"
#include "device_facts.hpp"
#include "lz4_frame_device.hiph"
#include "snappy_launch.hpp"

namespace hcamd {
namespace pqp {

using lz4f::block_scan;
using lz4f::groups;
using lz4f::kBlock;
using lz4f::kScanBlock;
using lz4f::kWavesPerBlock;
using lz4f::parts_of;
using lz4f::strided_copy;

namespace {

// the lists of a pass of P pages (parquet_pages_plan.hpp: kLists8 of 8-byte words, then kLists4 of 4-byte words)
struct Lists
{
  const uint8_t** comp_ptrs; // the batched decoder's five
  size_t* comp_bytes;
  uint8_t** out_ptrs;
  size_t* caps;
  size_t* actual;
  const uint8_t** stored_src; // the copy's three
  uint8_t** stored_dst;
  size_t* stored_bytes;
  const uint8_t** body_ptrs; // the chunk CRC kernel's two: 0 bytes where nothing is to be compared
  size_t* body_bytes;
  hipcompStatus_t* statuses;
  uint32_t* crcs;       // what the header says
  uint32_t* crc_values; // what the bytes say
  uint32_t* flags;      // kEntry*
  uint32_t* item_col;   // the item of the entry
};
static_assert(sizeof(hipcompStatus_t) == 4, "the statuses are a 4-byte list");
constexpr uint32_t kEntryDecoded = 1, kEntryChecked = 2;

Lists lists_of(uint8_t* s, uint64_t items, uint64_t P)
{
  Lists l;
  l.comp_ptrs = reinterpret_cast<const uint8_t**>(s + list8_at(items, P, 0));
  l.comp_bytes = reinterpret_cast<size_t*>(s + list8_at(items, P, 1));
  l.out_ptrs = reinterpret_cast<uint8_t**>(s + list8_at(items, P, 2));
  l.caps = reinterpret_cast<size_t*>(s + list8_at(items, P, 3));
  l.actual = reinterpret_cast<size_t*>(s + list8_at(items, P, 4));
  l.stored_src = reinterpret_cast<const uint8_t**>(s + list8_at(items, P, 5));
  l.stored_dst = reinterpret_cast<uint8_t**>(s + list8_at(items, P, 6));
  l.stored_bytes = reinterpret_cast<size_t*>(s + list8_at(items, P, 7));
  l.body_ptrs = reinterpret_cast<const uint8_t**>(s + list8_at(items, P, 8));
  l.body_bytes = reinterpret_cast<size_t*>(s + list8_at(items, P, 9));
  l.statuses = reinterpret_cast<hipcompStatus_t*>(s + list4_at(items, P, 0));
  l.crcs = reinterpret_cast<uint32_t*>(s + list4_at(items, P, 1));
  l.crc_values = reinterpret_cast<uint32_t*>(s + list4_at(items, P, 2));
  l.flags = reinterpret_cast<uint32_t*>(s + list4_at(items, P, 3));
  l.item_col = reinterpret_cast<uint32_t*>(s + list4_at(items, P, 4));
  return l;
}

// what a listing walk does with a page: a row of the table, an entry of the pass (lane 0)
struct ListSink
{
  Lists l;
  uint64_t at;       // of the item's first entry in the pass's lists
  Page* rows;        // where the item's rows of this pass go, or nullptr
  const uint8_t* in;
  uint8_t* out;
  uint64_t capacity;
  uint32_t item;
  bool worker, verify;
  __device__ __forceinline__ void page(uint64_t j, const Page& p)
  {
    // (the counting walk held the sum of the pages to the capacity: a page beyond it means the bytes changed under
    // the call; it stays the empty entry clear_kernel made, and list_kernel's count says the item failed)
    if (!worker || p.out_offset + p.uncompressed_page_size > capacity)
      return;
    if (rows)
      rows[j] = p;
    const uint64_t e = at + j, levels = levels_bytes(p), decoded = decoded_bytes(p);
    const bool checked = verify && (p.flags & kHasCrc);
    l.comp_ptrs[e] = in + p.body_offset + levels;
    l.comp_bytes[e] = decoded ? (size_t)compressed_bytes(p) : 0; // (0 bytes: the decoder looks at nothing)
    l.out_ptrs[e] = out + p.out_offset + levels;
    l.caps[e] = (size_t)decoded;
    l.actual[e] = 0;
    l.stored_src[e] = in + p.body_offset;
    l.stored_dst[e] = out + p.out_offset;
    l.stored_bytes[e] = (size_t)stored_bytes(p);
    l.body_ptrs[e] = in + p.body_offset;
    l.body_bytes[e] = checked ? (size_t)p.compressed_page_size : 0;
    l.statuses[e] = hipcompSuccess;
    l.crcs[e] = p.crc;
    l.crc_values[e] = 0;
    l.flags[e] = (decoded ? kEntryDecoded : 0u) | (checked ? kEntryChecked : 0u);
    l.item_col[e] = item;
  }
};

// wave w of the grid takes items w, w + waves, ...: all its lanes, on the same state
#define HC_ITEMS_OF_WAVE(it, num_items)                                                                                \
  for (uint64_t it = (uint64_t)blockIdx.x * kWavesPerBlock + uniform((uint32_t)(threadIdx.x >> 6)); it < (num_items);   \
       it += (uint64_t)gridDim.x * kWavesPerBlock)

// The counting walk.  items == nullptr: the size query, the answers go straight to the caller's arrays.
__global__ __launch_bounds__(kBlock) void count_kernel(Batch b, Item* items, size_t* q_pages, size_t* q_sizes,
                                                       hipcompStatus_t* q_statuses)
{
  const int lane = lane_id();
  HC_ITEMS_OF_WAVE(it, b.items)
  {
    const uint8_t* const p = uniform_ptr(b.chunk_ptrs[it]);
    const uint64_t n = uniform((uint64_t)b.chunk_bytes[it]);
    WindowSrc src(to_global(p), n, lane);
    NoSink none;
    const Walk w = walk_pages(src, n, b.codec, Walk(), ~uint64_t(0), none);
    if (lane != 0)
      continue;
    if (!items) {
      q_pages[it] = w.ok ? (size_t)w.pages : 0;
      q_sizes[it] = w.ok ? (size_t)w.out : 0;
      q_statuses[it] = w.ok ? hipcompSuccess : hipcompErrorCannotDecompress;
      continue;
    }
    Item z = {};
    z.in = p;
    z.n = n;
    z.out = b.out_ptrs[it];
    z.capacity = b.out_capacities[it];
    z.table = b.page_ptrs ? b.page_ptrs[it] : nullptr;
    z.fate = fate_of(w, b.page_ptrs != nullptr, b.page_ptrs ? (uint64_t)b.page_capacities[it] : 0, z.capacity);
    z.pages = z.fate == kFine ? w.pages : 0;
    z.total = z.fate == kFine ? w.out : 0;
    z.bare = w.bare;
    z.largest = w.largest;
    z.w = Walk();
    items[it] = z;
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
      v = items[i].pages;
      if (v && items[i].largest > mine)
        mine = items[i].largest;
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
    totals->pages = base;
    totals->largest = largest;
    totals->crc_sink = 0;
  }
}

// The listing walk of pass k: every item with pages in it takes its walk up where the last pass left it.
__global__ __launch_bounds__(kBlock) void list_kernel(Item* items, uint64_t num_items, Lists l, uint64_t P, uint64_t k, uint32_t codec,
                                                      bool verify)
{
  const int lane = lane_id();
  HC_ITEMS_OF_WAVE(it, num_items)
  {
    const uint64_t first = uniform(items[it].first), pages = uniform(items[it].pages);
    const Slice s = item_slice(first, pages, P, k);
    if (s.count == 0)
      continue;
    Walk w;
    w.pos = uniform(items[it].w.pos);
    w.out = uniform(items[it].w.out);
    w.pages = uniform(items[it].w.pages);
    const uint64_t before = w.pages, out_before = w.out;
    const uint8_t* const p = uniform_ptr(items[it].in);
    const uint64_t n = uniform(items[it].n);
    Page* const table = uniform_ptr(items[it].table);
    ListSink sink;
    sink.l = l;
    sink.at = s.at;
    sink.rows = table ? table + w.pages : nullptr;
    sink.in = p;
    sink.out = uniform_ptr(items[it].out);
    sink.capacity = uniform(items[it].capacity);
    sink.item = (uint32_t)it;
    sink.worker = lane == 0;
    sink.verify = verify;
    WindowSrc src(to_global(p), n, lane);
    w = walk_pages(src, n, codec, w, s.count, sink);
    if (lane == 0) {
      // (the counting walk read the same bytes: a walk that now stops short or leaves the capacity means they
      // changed under the call)
      if (!w.ok || w.pages - before != s.count || w.out > sink.capacity || w.out < out_before)
        atomicOr(&items[it].verdict, kVerdictCannotDecompress);
      items[it].w = w;
    }
  }
}

// an entry the listing walk did not reach (see above) is no entry: nothing of it is decoded, copied or compared
__global__ void clear_kernel(Lists l, uint32_t count)
{
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= count)
    return;
  l.comp_ptrs[e] = nullptr;
  l.comp_bytes[e] = 0;
  l.out_ptrs[e] = nullptr;
  l.caps[e] = 0;
  l.stored_bytes[e] = 0;
  l.body_ptrs[e] = nullptr;
  l.body_bytes[e] = 0;
  l.flags[e] = 0;
  l.item_col[e] = 0;
}

__global__ __launch_bounds__(kBlock) void stored_kernel(Lists l, uint32_t count)
{
  const uint32_t i = blockIdx.x;
  if (i >= count || l.stored_bytes[i] == 0)
    return;
  strided_copy(to_global(l.stored_dst[i]), to_global(l.stored_src[i]), l.stored_bytes[i], (uint64_t)blockIdx.y * kBlock + threadIdx.x,
               (uint64_t)gridDim.y * kBlock);
}

// what the batched decoder and the CRCs say of an entry, to its item's verdict word and to no other
__global__ void verdict_kernel(Item* items, Lists l, uint32_t count)
{
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= count)
    return;
  const uint32_t flags = l.flags[e];
  uint32_t verdict = 0;
  if ((flags & kEntryDecoded) && (l.statuses[e] != hipcompSuccess || l.actual[e] != l.caps[e]))
    verdict |= kVerdictCannotDecompress;
  if ((flags & kEntryChecked) && l.crc_values[e] != l.crcs[e])
    verdict |= kVerdictBadChecksum;
  if (verdict)
    atomicOr(&items[l.item_col[e]].verdict, verdict);
}

__global__ void finish_kernel(const Item* items, uint64_t num_items, bool require, size_t* sizes, hipcompStatus_t* statuses,
                              size_t* num_pages)
{
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= num_items)
    return;
  const uint32_t fate = items[i].fate, verdict = items[i].verdict;
  hipcompStatus_t status = hipcompSuccess;
  if (fate == kCannotDecompress)
    status = hipcompErrorCannotDecompress;
  else if (fate == kInvalidValue)
    status = hipcompErrorInvalidValue;
  else if (verdict & kVerdictBadChecksum)
    status = hipcompErrorBadChecksum;
  else if (verdict & kVerdictCannotDecompress)
    status = hipcompErrorCannotDecompress;
  else if (require && items[i].bare != 0)
    status = hipcompErrorCannotVerifyChecksums;
  const bool there = status == hipcompSuccess || status == hipcompErrorCannotVerifyChecksums;
  statuses[i] = status;
  sizes[i] = there ? (size_t)items[i].total : 0;
  num_pages[i] = there ? (size_t)items[i].pages : 0;
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

hipError_t launch_sizes(const Batch& b, size_t* num_pages, size_t* sizes, hipcompStatus_t* statuses, hipStream_t stream)
{
  count_kernel<<<walk_groups((const void*)count_kernel, b.items), kBlock, 0, stream>>>(b, nullptr, num_pages, sizes, statuses);
  return hipGetLastError();
}

#define HC_TRY(call)                                                                                                   \
  do {                                                                                                                 \
    const hipError_t e_ = (call);                                                                                      \
    if (e_ != hipSuccess)                                                                                              \
      return e_;                                                                                                       \
  } while (0)

hipError_t run(const Batch& b, size_t* actual_bytes, hipcompStatus_t* statuses, size_t* num_pages, uint8_t* scratch, uint64_t P,
               bool verify, bool require, hipStream_t stream, Stats* stats)
{
  Item* const items = reinterpret_cast<Item*>(scratch);
  Totals* const totals = reinterpret_cast<Totals*>(scratch + totals_at(b.items));
  const Lists l = lists_of(scratch, b.items, P);
  count_kernel<<<walk_groups((const void*)count_kernel, b.items), kBlock, 0, stream>>>(b, items, nullptr, nullptr, nullptr);
  HC_TRY(hipGetLastError());
  scan_items_kernel<<<1, kScanBlock, 0, stream>>>(items, b.items, totals);
  HC_TRY(hipGetLastError());
  Totals h;
  HC_TRY(hipMemcpyAsync(&h, totals, sizeof(h), hipMemcpyDeviceToHost, stream));
  HC_TRY(hipStreamSynchronize(stream));
  const uint64_t passes = passes_of(h.pages, P);
  if (stats) {
    stats->pages = h.pages;
    stats->passes = passes;
  }
  for (uint64_t k = 0; k < passes; ++k) {
    const uint32_t count = (uint32_t)pass_count(h.pages, P, k);
    clear_kernel<<<groups(count), kBlock, 0, stream>>>(l, count);
    HC_TRY(hipGetLastError());
    list_kernel<<<walk_groups((const void*)list_kernel, b.items), kBlock, 0, stream>>>(items, b.items, l, P, k, b.codec, verify);
    HC_TRY(hipGetLastError());
    if (b.codec == kCompressedColumn) {
      snappy_launch_decompress(l.comp_ptrs, l.comp_bytes, l.caps, count, l.out_ptrs, l.actual, l.statuses, stream);
      HC_TRY(hipGetLastError());
    }
    if (h.largest) { // (0: no page of the batch has a stored part)
      stored_kernel<<<dim3(count, parts_of(h.largest)), kBlock, 0, stream>>>(l, count);
      HC_TRY(hipGetLastError());
    }
    if (verify) {
      CrcChunks c;
      c.ptrs = l.body_ptrs;
      c.lens = l.body_bytes;
      c.count = count;
      CrcTarget t;
      t.values = l.crc_values;
      t.pass_bytes = uint64_t(1) << 32; // (no body is longer: the shift into the unread pass word does not wrap)
      t.pass_word = &totals->crc_sink;
      HC_TRY(crc_launch_chunks(c, t, stream));
    }
    verdict_kernel<<<groups(count), kBlock, 0, stream>>>(items, l, count);
    HC_TRY(hipGetLastError());
  }
  finish_kernel<<<groups(b.items), kBlock, 0, stream>>>(items, b.items, require, actual_bytes, statuses, num_pages);
  return hipGetLastError();
}

} // namespace pqp
} // namespace hcamd
