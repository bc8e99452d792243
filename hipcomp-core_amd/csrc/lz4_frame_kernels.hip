// lz4_frame_kernels.hip -- the kernels of the LZ4 manager's frame methods (lz4_frame_launch.hpp; the format and its
// arithmetic: lz4_frame.hpp, xxh32_math.hpp; the passes they make up: hlif.hip).
//
// Writing: the batched encoder fills a slot per chunk; a scan of the stored sizes continues from a cursor on the
// device, the block checksums are hashed, and the assembly kernel puts size word, bytes and checksum in place.
// Reading: one lane follows the block chain (each size word says where the next stands) and lists the blocks of a
// pass; sizes come from a parse, places from a scan; the batched decoder takes the compressed blocks of
// independent-block frames, a copy the stored ones, and a decoder that knows the frame's history -- one wave per
// frame, block after block -- those of linked-block frames.  Every store is a vector store.
// The device functions these kernels share with those of a batch of frames are in lz4_frame_device.hiph.
#include "lz4_frame_device.hiph"

namespace hcamd {
namespace lz4f {

namespace {

// ---- writing -------------------------------------------------------------------------------------------------
__global__ void write_header_kernel(uint8_t* frame, uint64_t content_size, uint32_t code, bool sums,
                                    unsigned long long* cursor)
{
  uint8_t h[kWrittenHeaderBytes];
  write_descriptor(h, code, content_size, sums);
  for (uint32_t k = 0; k < kWrittenHeaderBytes; ++k)
    frame[k] = h[k];
  *cursor = kWrittenHeaderBytes;
}

__global__ void write_lists_kernel(const uint8_t* in, uint64_t in_size, uint64_t chunk_bytes, uint64_t first,
                                   uint32_t count, uint8_t* slots, uint64_t slot_bytes, WriteLists l)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count)
    return;
  const uint64_t at = (first + i) * chunk_bytes;
  l.in_ptrs[i] = in + at;
  l.in_bytes[i] = (size_t)(in_size - at < chunk_bytes ? in_size - at : chunk_bytes);
  l.slots[i] = slots + (uint64_t)i * slot_bytes;
}

__global__ __launch_bounds__(kScanBlock) void write_scan_kernel(WriteLists l, uint32_t count, bool sums,
                                                                unsigned long long* cursor)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  uint64_t base = *cursor;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t i = tile + threadIdx.x;
    const uint64_t v = i < count ? block_bytes(l.stream_bytes[i], l.in_bytes[i], sums) : 0;
    uint64_t total;
    const uint64_t excl = block_scan(v, lds, total);
    if (i < count)
      l.offsets[i] = base + excl;
    base += total;
  }
  if (threadIdx.x == 0)
    *cursor = base;
}

__global__ void write_sums_kernel(WriteLists l, uint32_t count)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x, i = t >> 2;
  const bool on = i < count;
  const uint64_t chunk = on ? l.in_bytes[i] : 0, stream = on ? l.stream_bytes[i] : 0;
  const bool raw = stored(stream, chunk);
  cgptr p = to_global(on ? (raw ? l.in_ptrs[i] : l.slots[i]) : nullptr);
  const uint32_t h = quad_xxh32(p, on ? (raw ? chunk : stream) : 0, lane_id());
  if (on && (t & 3) == 0)
    l.sums[i] = h;
}

// block blockIdx.x of the pass, part blockIdx.y of gridDim.y of its bytes
__global__ __launch_bounds__(kBlock) void write_blocks_kernel(uint8_t* frame, WriteLists l, uint32_t count, bool sums)
{
  const uint32_t i = blockIdx.x;
  const uint64_t chunk = l.in_bytes[i], stream = l.stream_bytes[i];
  const bool raw = stored(stream, chunk);
  const uint64_t n = raw ? chunk : stream;
  gptr at = to_global(frame + l.offsets[i]);
  if (blockIdx.y == 0) {
    const uint32_t word = size_word(stream, chunk);
    if (threadIdx.x < 4)
      at[threadIdx.x] = (uint8_t)(word >> (8 * threadIdx.x));
    else if (sums && threadIdx.x < 8)
      at[4 + n + (threadIdx.x - 4)] = (uint8_t)(l.sums[i] >> (8 * (threadIdx.x - 4)));
  }
  strided_copy(at + 4, to_global(raw ? l.in_ptrs[i] : l.slots[i]), n, (uint64_t)blockIdx.y * kBlock + threadIdx.x,
               (uint64_t)gridDim.y * kBlock);
}

__global__ void write_end_kernel(uint8_t* frame, const unsigned long long* cursor, size_t* frame_bytes)
{
  const uint64_t at = *cursor;
  for (int k = 0; k < 4; ++k)
    frame[at + k] = 0;
  *frame_bytes = (size_t)(at + 4);
}

__global__ void set_size_kernel(size_t* word, size_t value) { *word = value; }

// ---- reading: the walk ---------------------------------------------------------------------------------------
__global__ void read_reset_kernel(ReadState* st)
{
  ReadState z = {};
  z.all_declared = 1;
  z.cur_content = kNoContentSize;
  *st = z;
}

__global__ void read_walk_kernel(const uint8_t* in, uint64_t n, ReadState* stp, ReadLists l, bool lists, uint32_t capacity,
                                 bool final, bool verify)
{
  read_walk(in, n, stp, l, lists, capacity, final, verify);
}

// The walk behind the passes of an indexed read (lz4_frame_index_launch.hpp): where they listed and placed everything,
// *skip says so and nothing is left to do here.  (A kernel of its own: the walk of a frame without an index is the
// kernel above, without a word to load and test.)
__global__ void read_walk_unless_kernel(const uint8_t* in, uint64_t n, ReadState* stp, ReadLists l, bool lists,
                                        uint32_t capacity, bool final, bool verify, const uint32_t* skip)
{
  if (*skip)
    return;
  read_walk(in, n, stp, l, lists, capacity, final, verify);
}

// ---- reading: sizes and places -------------------------------------------------------------------------------
// the decoded sizes of the compressed blocks of linked frames: one lane per block (linked_block_size)
__global__ void read_linked_sizes_kernel(ReadLists l, const ReadState* st)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count)
    return;
  const uint32_t flags = l.flags[i];
  if (!(flags & kLinked) || (flags & kStored))
    return;
  l.sizes[i] = linked_block_size(l.comp_ptrs[i], (uint32_t)l.comp_bytes[i]); // (at most the block maximum, 4 MiB)
}

__global__ __launch_bounds__(kScanBlock) void read_scan_kernel(ReadLists l, ReadState* st, uint8_t* out, uint64_t out_bytes)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  const uint32_t count = st->count;
  const uint64_t carried_start = st->frame_out_start;
  uint64_t base = st->out_cursor;
  bool bad = false;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t i = tile + threadIdx.x;
    uint64_t size = 0;
    uint32_t flags = 0;
    if (i < count) {
      flags = l.flags[i];
      size = (flags & kStored) ? l.comp_bytes[i] : (flags & kLinked) ? l.sizes[i] : l.actual[i];
      if (size > block_max_of_code((flags >> 8) & 7u)) {
        bad = true;
        size = 0;
      }
    }
    uint64_t total;
    const uint64_t off = base + block_scan(size, lds, total);
    if (i < count) {
      if (off > out_bytes || size > out_bytes - off) { // no room: the block gets none
        bad = true;
        size = 0;
      }
      l.sizes[i] = (size_t)size;
      l.out_ptrs[i] = out + (off < out_bytes ? off : out_bytes);
      l.caps[i] = (size_t)size;
      l.batch_caps[i] = (flags & (kStored | kLinked)) ? 0 : (size_t)size;
    }
    base += total;
  }
  __syncthreads();
  // a frame that ends in this pass and declares its size: from its first byte to its last block's end
  for (uint32_t i = threadIdx.x; i < count; i += kScanBlock) {
    if (!(l.flags[i] & kLast) || l.aux[i] == kNoContentSize)
      continue;
    const int32_t head = l.head[i];
    const uint64_t start = head >= 0 ? (uint64_t)(l.out_ptrs[head] - out) : carried_start;
    const uint64_t end = (uint64_t)(l.out_ptrs[i] - out) + l.caps[i];
    if (end - start != l.aux[i])
      bad = true;
  }
  if (bad)
    atomicOr(&st->verdict, kVerdictCannotDecompress);
  __syncthreads();
  if (threadIdx.x == 0)
    st->out_cursor = base;
}

// ---- reading: the blocks -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void read_stored_kernel(ReadLists l, const ReadState* st)
{
  const uint32_t i = blockIdx.x;
  if (i >= st->count || !(l.flags[i] & kStored))
    return;
  strided_copy(to_global(l.out_ptrs[i]), to_global(l.comp_ptrs[i]), l.caps[i], (uint64_t)blockIdx.y * kBlock + threadIdx.x,
               (uint64_t)gridDim.y * kBlock);
}

// one wave per linked frame of the pass (linked_frame_of_wave)
__global__ __launch_bounds__(kBlock) void read_linked_kernel(ReadLists l, ReadState* st, uint8_t* out_base)
{
  linked_frame_of_wave(l, st->count, OneRead{st, out_base});
}

__global__ void read_verdict_kernel(ReadLists l, ReadState* st)
{
  batched_verdict_of_thread(l, st->count, OneRead{st, nullptr});
}

__global__ void read_block_sums_kernel(ReadLists l, ReadState* st)
{
  block_sum_of_quad(l, st->count, OneRead{st, nullptr});
}

__global__ __launch_bounds__(kBlock) void read_content_sums_kernel(ReadLists l, ReadState* st, uint8_t* out)
{
  content_sum_of_wave(l, st->count, OneRead{st, out});
}

__global__ void read_pass_end_kernel(ReadLists l, ReadState* st, uint8_t* out)
{
  const uint32_t count = st->count;
  if (count == 0)
    return;
  const int32_t head = l.head[count - 1];
  if (head >= 0)
    st->frame_out_start = (uint64_t)(l.out_ptrs[head] - out);
}

__global__ void read_finish_kernel(const ReadState* st, uint64_t num_blocks, uint64_t out_bytes, bool require,
                                   hipcompStatus_t* status)
{
  if (st->verdict & kVerdictBadChecksum)
    *status = hipcompErrorBadChecksum;
  else if (st->reason != kOk)
    *status = (hipcompStatus_t)status_of(st->reason);
  else if ((st->verdict & kVerdictCannotDecompress) || !st->done || st->blocks != num_blocks || st->out_cursor != out_bytes)
    *status = hipcompErrorCannotDecompress;
  else if (require && st->bare_frames != 0)
    *status = hipcompErrorCannotVerifyChecksums;
  else
    *status = hipcompSuccess;
}

} // namespace

hipError_t launch_write_header(uint8_t* frame, uint64_t content_size, uint32_t block_max_code, bool block_checksums,
                               unsigned long long* cursor, hipStream_t stream)
{
  write_header_kernel<<<1, 1, 0, stream>>>(frame, content_size, block_max_code, block_checksums, cursor);
  return hipGetLastError();
}

hipError_t launch_write_lists(const uint8_t* in, uint64_t in_size, uint64_t chunk_bytes, uint64_t first, uint32_t count,
                              uint8_t* slots, uint64_t slot_bytes, const WriteLists& l, hipStream_t stream)
{
  write_lists_kernel<<<groups(count), kBlock, 0, stream>>>(in, in_size, chunk_bytes, first, count, slots, slot_bytes, l);
  return hipGetLastError();
}

hipError_t launch_write_scan(const WriteLists& l, uint32_t count, bool block_checksums, unsigned long long* cursor,
                             hipStream_t stream)
{
  write_scan_kernel<<<1, kScanBlock, 0, stream>>>(l, count, block_checksums, cursor);
  return hipGetLastError();
}

hipError_t launch_write_sums(const WriteLists& l, uint32_t count, hipStream_t stream)
{
  write_sums_kernel<<<groups(4ull * count), kBlock, 0, stream>>>(l, count);
  return hipGetLastError();
}

hipError_t launch_write_blocks(uint8_t* frame, const WriteLists& l, uint32_t count, uint64_t chunk_bytes,
                               bool block_checksums, hipStream_t stream)
{
  write_blocks_kernel<<<dim3(count, parts_of(chunk_bytes)), kBlock, 0, stream>>>(frame, l, count, block_checksums);
  return hipGetLastError();
}

hipError_t launch_write_end(uint8_t* frame, const unsigned long long* cursor, size_t* frame_bytes, hipStream_t stream)
{
  write_end_kernel<<<1, 1, 0, stream>>>(frame, cursor, frame_bytes);
  return hipGetLastError();
}

hipError_t launch_set_size(size_t* word, size_t value, hipStream_t stream)
{
  set_size_kernel<<<1, 1, 0, stream>>>(word, value);
  return hipGetLastError();
}

hipError_t launch_read_reset(ReadState* st, hipStream_t stream)
{
  read_reset_kernel<<<1, 1, 0, stream>>>(st);
  return hipGetLastError();
}

hipError_t launch_read_walk(const uint8_t* in, uint64_t in_bytes, ReadState* st, const ReadLists* lists, uint32_t capacity,
                            bool verify, hipStream_t stream, const uint32_t* skip)
{
  if (skip)
    read_walk_unless_kernel<<<1, 1, 0, stream>>>(in, in_bytes, st, lists ? *lists : ReadLists(), lists != nullptr, capacity,
                                                 lists != nullptr && capacity == 0, verify, skip);
  else
    read_walk_kernel<<<1, 1, 0, stream>>>(in, in_bytes, st, lists ? *lists : ReadLists(), lists != nullptr, capacity,
                                          lists != nullptr && capacity == 0, verify);
  return hipGetLastError();
}

hipError_t launch_read_linked_sizes(const ReadLists& l, const ReadState* st, uint32_t capacity, hipStream_t stream)
{
  read_linked_sizes_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_scan(const ReadLists& l, ReadState* st, uint32_t, uint8_t* out, uint64_t out_bytes, hipStream_t stream)
{
  read_scan_kernel<<<1, kScanBlock, 0, stream>>>(l, st, out, out_bytes);
  return hipGetLastError();
}

hipError_t launch_read_stored(const ReadLists& l, const ReadState* st, uint32_t capacity, uint64_t largest_block,
                              hipStream_t stream)
{
  read_stored_kernel<<<dim3(capacity, parts_of(largest_block)), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_linked(const ReadLists& l, ReadState* st, uint32_t capacity, uint8_t* out, hipStream_t stream)
{
  read_linked_kernel<<<groups((uint64_t)capacity * kWave), kBlock, 0, stream>>>(l, st, out);
  return hipGetLastError();
}

hipError_t launch_read_verdict(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream)
{
  read_verdict_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_block_sums(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream)
{
  read_block_sums_kernel<<<groups(4ull * capacity), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_content_sums(const ReadLists& l, ReadState* st, uint32_t capacity, uint8_t* out, hipStream_t stream)
{
  read_content_sums_kernel<<<groups((uint64_t)capacity * kWave), kBlock, 0, stream>>>(l, st, out);
  return hipGetLastError();
}

hipError_t launch_read_pass_end(const ReadLists& l, ReadState* st, uint8_t* out, hipStream_t stream)
{
  read_pass_end_kernel<<<1, 1, 0, stream>>>(l, st, out);
  return hipGetLastError();
}

hipError_t launch_read_finish(const ReadState* st, uint64_t num_blocks, uint64_t out_bytes, bool require_checksums,
                              hipcompStatus_t* status, hipStream_t stream)
{
  read_finish_kernel<<<1, 1, 0, stream>>>(st, num_blocks, out_bytes, require_checksums, status);
  return hipGetLastError();
}

} // namespace lz4f
} // namespace hcamd
