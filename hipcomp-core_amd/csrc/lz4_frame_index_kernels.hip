// lz4_frame_index_kernels.hip -- the kernels of seekable LZ4 frames (lz4_frame_index_launch.hpp; the index and the
// tests it has to pass: lz4_frame_index.hpp; the passes: hlif.hip).
//
// Writing: the fields, the size words of every pass (the words write_blocks_kernel puts into the frame, from the
// same lists) and, once they all stand, the hash.  Reading: one workgroup hops from frame to frame -- per frame
// one lane reads the fields and the descriptor, the workgroup sums the block lengths, a wave hashes -- and one
// workgroup per pass scans the lengths from a cursor on the device, gathers the size word at every scanned offset
// and writes the entries the chain's walk, the parse-only pass and the placing scan would have written.  The index
// is untrusted: every address is tested against the input's length before it is read.  Every store is a vector
// store.
#include "lz4_frame_index_launch.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace lz4f {

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;

// exclusive scan over the kScanBlock threads of a workgroup; total: the sum (lz4_frame_kernels.hip has the same)
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* lds, uint64_t& total)
{
  const uint64_t incl = wave_scan_add_u64(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63)
    lds[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t run = 0;
    for (int w = 0; w < kScanBlock / kWave; ++w) {
      const uint64_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[kScanBlock / kWave] = run;
  }
  __syncthreads();
  const uint64_t excl = incl - v + lds[wave];
  total = lds[kScanBlock / kWave];
  __syncthreads();
  return excl;
}

// XXH32 (seed 0) of len bytes at p by a whole wave; every lane returns the hash.  The four accumulators are four
// chains by the construction of the hash; what a wave adds is the loading: lane t takes the dword at 4t of a
// 256-byte tile (16 stripes), four tiles at a time and the next four while these are worked in, and the chains
// read their words across the lanes (lane `sub` of a quad stands for accumulator `sub`, as in quad_xxh32).
__device__ uint32_t wave_xxh32(cgptr p, uint64_t len, int lane)
{
  const int sub = lane & 3;
  uint32_t acc = xxh32::acc_init(sub, 0);
  const uint64_t stripes = len >> 4;
  uint64_t s = 0;
  if (stripes >= 64) {
    cgptr q = p + 4 * lane;
    uint32_t w0 = load_u32_any(q), w1 = load_u32_any(q + 256), w2 = load_u32_any(q + 512), w3 = load_u32_any(q + 768);
    for (; s + 64 <= stripes; s += 64) {
      const bool more = s + 128 <= stripes; // (wave-uniform)
      uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
      if (more) {
        cgptr r = p + 16 * (s + 64) + 4 * lane;
        n0 = load_u32_any(r);
        n1 = load_u32_any(r + 256);
        n2 = load_u32_any(r + 512);
        n3 = load_u32_any(r + 768);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        acc = xxh32::round(acc, (uint32_t)__shfl((int)w0, 4 * j + sub));
#pragma unroll
      for (int j = 0; j < 16; ++j)
        acc = xxh32::round(acc, (uint32_t)__shfl((int)w1, 4 * j + sub));
#pragma unroll
      for (int j = 0; j < 16; ++j)
        acc = xxh32::round(acc, (uint32_t)__shfl((int)w2, 4 * j + sub));
#pragma unroll
      for (int j = 0; j < 16; ++j)
        acc = xxh32::round(acc, (uint32_t)__shfl((int)w3, 4 * j + sub));
      w0 = n0;
      w1 = n1;
      w2 = n2;
      w3 = n3;
    }
  }
  for (; s < stripes; ++s)
    acc = xxh32::round(acc, load_u32_any(p + 16 * s + 4 * sub));
  const uint32_t v1 = (uint32_t)__shfl((int)acc, 0), v2 = (uint32_t)__shfl((int)acc, 1), v3 = (uint32_t)__shfl((int)acc, 2),
                 v4 = (uint32_t)__shfl((int)acc, 3);
  uint32_t h = stripes ? xxh32::merge(v1, v2, v3, v4) : xxh32::short_init(0);
  h += (uint32_t)len;
  cgptr r = p + (stripes << 4);
  uint32_t rest = (uint32_t)(len & 15u);
  for (; rest >= 4; rest -= 4, r += 4)
    h = xxh32::tail_word(h, load_u32_any(r));
  for (; rest; --rest, ++r)
    h = xxh32::tail_byte(h, *r);
  return xxh32::avalanche(h);
}

// ---- writing -------------------------------------------------------------------------------------------------
__global__ void index_write_fields_kernel(uint8_t* index, uint32_t blocks, uint32_t block_bytes, uint64_t content_bytes,
                                          bool sums)
{
  uint8_t h[kIndexWordsAt];
  write_index_fields(h, blocks, block_bytes, content_bytes, sums);
  for (uint32_t k = 0; k < kIndexWordsAt; ++k)
    index[k] = h[k];
}

__global__ void index_write_words_kernel(uint8_t* index, WriteLists l, uint64_t first, uint32_t count)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count)
    return;
  store_u32_any(to_global(index) + kIndexWordsAt + 4 * (first + i), size_word(l.stream_bytes[i], l.in_bytes[i]));
}

__global__ __launch_bounds__(kWave) void index_write_end_kernel(uint8_t* index, uint32_t blocks, size_t* frame_bytes)
{
  const int lane = lane_id();
  const uint64_t hashed = 32 + 4 * (uint64_t)blocks;
  const uint32_t h = wave_xxh32(to_global(index) + 8, hashed, lane);
  if (lane == 0) {
    store_u32_any(to_global(index) + 8 + hashed, h);
    *frame_bytes += (size_t)index_bytes(blocks);
  }
}

// ---- reading: from frame to frame ----------------------------------------------------------------------------
struct Hop // what one lane finds in front of a frame, for the workgroup
{
  uint32_t reason; // of the fields and the descriptor
  uint32_t stop;   // the end of the input, or a refusal: no frame to work on
  IndexedEntry e;
  uint64_t index_at;
};

__global__ __launch_bounds__(kScanBlock) void index_begin_kernel(const uint8_t* in, uint64_t n, IndexState* ix)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  __shared__ Hop hop;
  __shared__ uint32_t hash;
  uint64_t pos = 0, blocks = 0, content = 0;
  uint32_t frames = 0, bare = 0, reason = kIndexOk;
  for (;;) {
    if (threadIdx.x == 0) {
      hop.stop = 0;
      hop.reason = kIndexOk;
      // skippable frames of other magics
      while (n - pos >= 8 && is_skippable(xxh32::read32(in + pos)) && xxh32::read32(in + pos) != kIndexMagic) {
        const uint64_t size = xxh32::read32(in + pos + 4);
        if (size > n - pos - 8) {
          hop.reason = kIndexNotThere;
          break;
        }
        pos += 8 + size;
      }
      if (hop.reason != kIndexOk || pos == n) {
        hop.stop = 1;
      } else {
        IndexHead h;
        Descriptor d;
        uint32_t r = parse_index_fields(in + pos, n - pos, h);
        if (r == kIndexOk)
          r = check_indexed_descriptor(h, in + pos + index_bytes(h.blocks), n - pos - index_bytes(h.blocks), d);
        if (r == kIndexOk && (frames == kMaxIndexedFrames || blocks + h.blocks > 0xFFFFFFFFull))
          r = kIndexTooManyFrames;
        hop.reason = r;
        hop.stop = r != kIndexOk;
        if (r == kIndexOk) {
          hop.index_at = pos;
          hop.e.words_at = pos + kIndexWordsAt;
          hop.e.blocks_at = pos + index_bytes(h.blocks) + d.header_bytes;
          hop.e.first_block = blocks;
          hop.e.out_start = content;
          hop.e.content_bytes = h.content_bytes;
          hop.e.blocks = h.blocks;
          hop.e.block_bytes = h.block_bytes;
          hop.e.flags = (h.block_checksums() ? kBlockSum : 0u) | (code_for_chunk(d.block_max) << 8);
          hop.e.reserved = 0;
        }
      }
    }
    __syncthreads();
    if (hop.stop) {
      reason = hop.reason;
      break;
    }
    const IndexedEntry e = hop.e;
    const uint64_t index_at = hop.index_at;
    const bool sums = e.flags & kBlockSum;
    // the bytes of the blocks: the words lie inside the input (parse_index_fields: the payload does)
    uint64_t v = 0;
    for (uint64_t i = threadIdx.x; i < e.blocks; i += kScanBlock)
      v += indexed_block_bytes(load_u32_any(to_global(in) + e.words_at + 4 * i), sums);
    uint64_t total;
    block_scan(v, lds, total);
    if (threadIdx.x < kWave) {
      const uint32_t h = wave_xxh32(to_global(in) + index_at + 8, 32 + 4 * (uint64_t)e.blocks, lane_id());
      if (threadIdx.x == 0)
        hash = h;
    }
    __syncthreads();
    // (every thread comes to the same verdict)
    const uint64_t end_at = e.blocks_at + total;
    if (hash != xxh32::read32(in + e.words_at + 4 * (uint64_t)e.blocks))
      reason = kIndexHash;
    else if (end_at > n || n - end_at < 4)
      reason = kIndexOffset;
    else if (!is_end_mark(xxh32::read32(in + end_at)))
      reason = kIndexEndMark;
    if (reason != kIndexOk)
      break;
    if (threadIdx.x == 0)
      ix->frame[frames] = e;
    frames += 1;
    bare += sums ? 0 : 1;
    blocks += e.blocks;
    content += e.content_bytes;
    pos = end_at + 4;
    __syncthreads(); // (hop is written again)
  }
  if (threadIdx.x == 0) {
    ix->ok = reason == kIndexOk && frames != 0;
    ix->reason = reason == kIndexOk && frames == 0 ? (uint32_t)kIndexNotThere : reason;
    ix->skip = 0;
    ix->frames = frames;
    ix->blocks = blocks;
    ix->content_bytes = content;
    ix->listed = 0;
    ix->cursor = 0;
    ix->cur = 0;
    ix->bare_frames = bare;
  }
}

// ---- reading: the entries of a pass --------------------------------------------------------------------------
__device__ __forceinline__ void ask_nothing(const ReadLists& l, uint32_t capacity)
{
  for (uint32_t i = threadIdx.x; i < capacity; i += blockDim.x) {
    l.batch_bytes[i] = 0;
    l.batch_caps[i] = 0;
  }
}

__global__ __launch_bounds__(kScanBlock) void index_list_kernel(const uint8_t* in, uint64_t n, IndexState* ix, ReadState* st,
                                                                ReadLists l, bool lists, uint32_t capacity, uint8_t* out,
                                                                uint64_t out_bytes)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  __shared__ uint32_t refused;
  if (threadIdx.x == 0)
    refused = kIndexOk;
  __syncthreads();
  if (!ix->ok) {
    if (lists)
      ask_nothing(l, capacity);
    if (threadIdx.x == 0)
      st->count = 0;
    return;
  }
  const uint64_t before = ix->listed, all = ix->blocks;
  // (a caller that asks for more blocks than the frames hold: not this path's business, the chain's reader says so)
  const uint64_t want = lists ? (uint64_t)capacity : all - before;
  uint32_t cur = ix->cur;
  uint64_t cursor = ix->cursor, listed = 0;
  uint32_t why = all - before < want ? (uint32_t)kIndexCount : (uint32_t)kIndexOk;
  cgptr gin = to_global(in);
  while (why == kIndexOk && listed < want) {
    const IndexedEntry f = ix->frame[cur];
    const uint64_t b0 = before + listed - f.first_block; // the frame's first block of this pass
    const uint64_t left = f.blocks - b0, room = want - listed;
    const uint64_t take = left < room ? left : room;
    const bool sums = f.flags & kBlockSum;
    uint64_t base = b0 == 0 ? f.blocks_at : cursor;
    for (uint64_t tile = 0; tile < take; tile += kScanBlock) {
      const uint64_t i = tile + threadIdx.x, b = b0 + i;
      const bool on = i < take;
      const uint32_t word = on ? load_u32_any(gin + f.words_at + 4 * b) : 0;
      const uint64_t bytes = on ? indexed_block_bytes(word, sums) : 0;
      uint64_t total;
      const uint64_t off = base + block_scan(bytes, lds, total);
      if (on) {
        const uint64_t content = b + 1 < f.blocks ? f.block_bytes : f.content_bytes - (uint64_t)f.block_bytes * b;
        const uint64_t place = f.out_start + (uint64_t)f.block_bytes * b;
        // the block with its size word (and checksum) inside the input, its content inside the output
        if (off > n || n - off < bytes)
          why = kIndexOffset;
        else if (lists && (place > out_bytes || out_bytes - place < content))
          why = kIndexOffset;
        else
          why = check_indexed_block(word, load_u32_any(gin + off), content, f.block_bytes);
        if (why == kIndexOk && lists) {
          const uint64_t e = listed + i;
          const uint64_t len = word & ~kStoredBit;
          const bool raw = word & kStoredBit;
          l.comp_ptrs[e] = in + off + 4;
          l.comp_bytes[e] = (size_t)len;
          l.batch_bytes[e] = raw ? 0 : (size_t)len;
          l.sizes[e] = (size_t)content;
          l.out_ptrs[e] = out + place;
          l.caps[e] = (size_t)content;
          l.batch_caps[e] = raw ? 0 : (size_t)content;
          l.aux[e] = kNoContentSize;
          l.flags[e] = f.flags | (raw ? kStored : 0u) | (b + 1 == f.blocks ? kLast : 0u);
          l.head[e] = -1;
        }
        if (why != kIndexOk)
          atomicMax(&refused, why);
      }
      base += total;
    }
    cursor = base;
    listed += take;
    if (b0 + take == f.blocks) {
      // the EndMark behind the frame's last block (index_begin_kernel found it behind the sum of the lengths: here
      // that sum is the one of lengths that were each found in their place)
      if (cursor > n || n - cursor < 4 || !is_end_mark(load_u32_any(gin + cursor)))
        atomicMax(&refused, (uint32_t)kIndexEndMark);
      cur += 1;
    }
    __syncthreads();
    why = refused;
  }
  __syncthreads();
  if (why == kIndexOk)
    why = refused;
  if (why != kIndexOk) {
    if (lists)
      ask_nothing(l, capacity);
    if (threadIdx.x == 0) {
      ix->ok = 0;
      ix->reason = why;
      st->count = 0;
    }
    return;
  }
  if (threadIdx.x == 0) {
    ix->listed = before + listed;
    ix->cursor = cursor;
    ix->cur = cur;
    st->count = lists ? (uint32_t)listed : 0;
  }
}

__global__ void index_verdict_kernel(ReadLists l, const ReadState* st, IndexState* ix)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count || (l.flags[i] & kStored))
    return;
  if (l.statuses[i] != hipcompSuccess || l.actual[i] != l.caps[i]) {
    ix->reason = kIndexDecode;
    ix->ok = 0;
  }
}

__global__ void index_end_kernel(IndexState* ix, ReadState* st, ReadLists l, uint32_t capacity, uint64_t n, uint64_t num_blocks)
{
  // (ok, listed and blocks are not written here: every thread reads the same)
  const bool held = ix->ok && ix->listed == ix->blocks && ix->blocks == num_blocks;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (held && i < capacity) {
    l.batch_bytes[i] = 0;
    l.batch_caps[i] = 0;
  }
  if (i != 0)
    return;
  ix->skip = held;
  if (held) {
    st->pos = n;
    st->blocks = ix->blocks;
    st->frames = ix->frames;
    st->declared_sum = ix->content_bytes;
    st->out_cursor = ix->content_bytes;
    st->bare_frames = ix->bare_frames;
    st->in_frame = 0;
    st->done = 1;
    st->count = 0;
  } else {
    ReadState z = {};
    z.all_declared = 1;
    z.cur_content = kNoContentSize;
    *st = z;
  }
}

// ---- ranged reads ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanBlock) void index_range_list_kernel(const uint8_t* in, uint64_t n, const IndexState* ix,
                                                                      uint32_t frame, range::Plan plan, uint64_t pass_first,
                                                                      uint32_t count, uint8_t* out, RangeSlots slots, ReadLists l,
                                                                      ReadState* st)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  const IndexedEntry f = ix->frame[frame];
  const bool sums = f.flags & kBlockSum;
  cgptr gin = to_global(in);
  // where block pass_first stands: behind the blocks before it
  uint64_t v = 0, total;
  for (uint64_t b = threadIdx.x; b < pass_first; b += kScanBlock)
    v += indexed_block_bytes(load_u32_any(gin + f.words_at + 4 * b), sums);
  block_scan(v, lds, total);
  uint64_t base = f.blocks_at + total;
  bool bad = false;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t i = tile + threadIdx.x;
    const bool on = i < count;
    const uint64_t b = pass_first + i;
    const uint32_t word = on ? load_u32_any(gin + f.words_at + 4 * b) : 0;
    const uint64_t bytes = on ? indexed_block_bytes(word, sums) : 0;
    const uint64_t off = base + block_scan(bytes, lds, total);
    if (on) {
      const range::Span s = range::range_span(plan, b, pass_first);
      // (launch_index_list has tested every block of this input in its place: a block that lies outside it now is
      // another input's, and asks nothing)
      const bool inside = off <= n && n - off >= bytes;
      const uint64_t len = inside ? word & ~kStoredBit : 0;
      const bool raw = word & kStoredBit;
      bad = bad || !inside;
      l.comp_ptrs[i] = inside ? in + off + 4 : in;
      l.comp_bytes[i] = (size_t)len;
      l.batch_bytes[i] = raw ? 0 : (size_t)len;
      l.sizes[i] = (size_t)s.cap;
      l.out_ptrs[i] = s.edge ? slots.base + (uint64_t)s.slot * slots.stride : out + s.dst_at;
      l.caps[i] = inside ? (size_t)s.cap : 0;
      l.batch_caps[i] = raw || !inside ? 0 : (size_t)s.cap;
      l.aux[i] = kNoContentSize;
      l.flags[i] = inside ? f.flags | (raw ? kStored : 0u) : kStored;
      l.head[i] = -1;
    }
    base += total;
  }
  if (bad)
    atomicOr(&st->verdict, kVerdictCannotDecompress);
  if (threadIdx.x == 0)
    st->count = count;
}

__global__ void index_range_settle_kernel(ReadLists l, const ReadState* st)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count || !(l.flags[i] & kStored))
    return;
  l.statuses[i] = hipcompSuccess;
  l.actual[i] = l.caps[i];
}

__global__ void index_range_finish_kernel(const ReadState* st, bool cannot_verify, hipcompStatus_t* status)
{
  if (st->verdict & kVerdictBadChecksum)
    *status = hipcompErrorBadChecksum;
  else if (st->verdict & kVerdictCannotDecompress)
    *status = hipcompErrorCannotDecompress;
  else if (cannot_verify)
    *status = hipcompErrorCannotVerifyChecksums;
  else
    *status = hipcompSuccess;
}

inline uint32_t groups(uint64_t threads) { return (uint32_t)((threads + kBlock - 1) / kBlock); }

} // namespace

hipError_t launch_index_write_fields(uint8_t* index, uint32_t blocks, uint32_t block_bytes, uint64_t content_bytes,
                                     bool block_checksums, hipStream_t stream)
{
  index_write_fields_kernel<<<1, 1, 0, stream>>>(index, blocks, block_bytes, content_bytes, block_checksums);
  return hipGetLastError();
}

hipError_t launch_index_write_words(uint8_t* index, const WriteLists& l, uint64_t first, uint32_t count, hipStream_t stream)
{
  index_write_words_kernel<<<groups(count), kBlock, 0, stream>>>(index, l, first, count);
  return hipGetLastError();
}

hipError_t launch_index_write_end(uint8_t* index, uint32_t blocks, size_t* frame_bytes, hipStream_t stream)
{
  index_write_end_kernel<<<1, kWave, 0, stream>>>(index, blocks, frame_bytes);
  return hipGetLastError();
}

hipError_t launch_index_begin(const uint8_t* in, uint64_t in_bytes, IndexState* ix, hipStream_t stream)
{
  index_begin_kernel<<<1, kScanBlock, 0, stream>>>(in, in_bytes, ix);
  return hipGetLastError();
}

hipError_t launch_index_list(const uint8_t* in, uint64_t in_bytes, IndexState* ix, ReadState* st, const ReadLists* lists,
                             uint32_t capacity, uint8_t* out, uint64_t out_bytes, hipStream_t stream)
{
  index_list_kernel<<<1, kScanBlock, 0, stream>>>(in, in_bytes, ix, st, lists ? *lists : ReadLists(), lists != nullptr,
                                                  capacity, out, out_bytes);
  return hipGetLastError();
}

hipError_t launch_index_verdict(const ReadLists& l, const ReadState* st, IndexState* ix, uint32_t capacity, hipStream_t stream)
{
  index_verdict_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, st, ix);
  return hipGetLastError();
}

hipError_t launch_index_end(IndexState* ix, ReadState* st, const ReadLists& l, uint32_t capacity, uint64_t in_bytes,
                            uint64_t num_blocks, hipStream_t stream)
{
  index_end_kernel<<<groups(capacity ? capacity : 1), kBlock, 0, stream>>>(ix, st, l, capacity, in_bytes, num_blocks);
  return hipGetLastError();
}

hipError_t launch_index_range_list(const uint8_t* in, uint64_t in_bytes, const IndexState* ix, uint32_t frame,
                                   const range::Plan& plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                                   const RangeSlots& slots, const ReadLists& l, ReadState* st, hipStream_t stream)
{
  index_range_list_kernel<<<1, kScanBlock, 0, stream>>>(in, in_bytes, ix, frame, plan, pass_first, count, out, slots, l, st);
  return hipGetLastError();
}

hipError_t launch_index_range_settle(const ReadLists& l, const ReadState* st, uint32_t capacity, hipStream_t stream)
{
  index_range_settle_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_index_range_finish(const ReadState* st, bool cannot_verify, hipcompStatus_t* status, hipStream_t stream)
{
  index_range_finish_kernel<<<1, 1, 0, stream>>>(st, cannot_verify, status);
  return hipGetLastError();
}

} // namespace lz4f
} // namespace hcamd
