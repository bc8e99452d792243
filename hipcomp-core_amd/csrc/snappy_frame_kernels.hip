// snappy_frame_kernels.hip -- the kernels of the Snappy manager's framed-stream methods (snappy_frame_launch.hpp;
// the format and its arithmetic: snappy_frame.hpp, crc32c_math.hpp; the passes they make up: hlif.hip).
//
// Writing: the batched encoder fills a slot per chunk; the input chunks' CRC-32C are computed one wave per chunk, a
// scan of the written sizes continues from a cursor on the device, and the assembly kernel puts header, masked CRC
// and bytes -- the slot's or the input's -- in place.
// Reading: one lane follows the chunk chain (each header says where the next stands; the format has no index) and
// lists the data chunks of a pass with what their first 13 bytes say: payload, kind, stored CRC, output bytes.
// Places come from a scan; the batched decoder takes the compressed chunks, a copy the stored ones, and the CRC
// kernel compares.  Every store is a vector store.
#include "device_facts.hpp"
#include "snappy_frame_device.hiph"
#include "snappy_frame_launch.hpp"

namespace hcamd {
namespace szf {

namespace {

// ---- shared pieces -------------------------------------------------------------------------------------------
// n bytes dst <- src by `threads` threads, this one number t: 16-byte aligned stores, 16-byte loads wherever they
// lie, single bytes in front of the first and behind the last aligned block (range_kernels.hip has the same loop)
__device__ __forceinline__ void strided_copy(gptr dst, cgptr src, uint64_t n, uint64_t t, uint64_t threads)
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

// ---- writing -------------------------------------------------------------------------------------------------
__global__ void write_begin_kernel(uint8_t* frame, unsigned long long* cursor)
{
  if (threadIdx.x < kIdentifierBytes)
    frame[threadIdx.x] = (uint8_t)identifier().byte(threadIdx.x);
  if (threadIdx.x == 0)
    *cursor = kIdentifierBytes;
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

// one wave per chunk, grid-stride over the pass
__global__ __launch_bounds__(kBlock) void write_crcs_kernel(WriteLists l, uint32_t count)
{
  __shared__ LdsTables L;
  fill_tables(L);
  const int lane = lane_id();
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  for (uint32_t i = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; i < count; i += waves) {
    const uint32_t crc = wave_crc(L, l.in_ptrs[i], (uint32_t)l.in_bytes[i], lane);
    if (lane == 0)
      l.crcs[i] = mask_crc(crc);
  }
}

__global__ __launch_bounds__(kScanBlock) void write_scan_kernel(WriteLists l, uint32_t count, unsigned long long* cursor)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  uint64_t base = *cursor;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t i = tile + threadIdx.x;
    const uint64_t v = i < count ? written_bytes(l.block_bytes[i], l.in_bytes[i]) : 0;
    uint64_t total;
    const uint64_t excl = block_scan(v, lds, total);
    if (i < count)
      l.offsets[i] = base + excl;
    base += total;
  }
  if (threadIdx.x == 0)
    *cursor = base;
}

// chunk blockIdx.x of the pass, part blockIdx.y of gridDim.y of its bytes
__global__ __launch_bounds__(kBlock) void write_chunks_kernel(uint8_t* frame, WriteLists l, uint32_t count)
{
  const uint32_t i = blockIdx.x;
  const uint64_t chunk = l.in_bytes[i], block = l.block_bytes[i];
  const bool raw = stored(block, chunk);
  gptr at = to_global(frame + l.offsets[i]);
  if (blockIdx.y == 0 && threadIdx.x < kDataHeaderBytes) {
    const uint32_t word = threadIdx.x < 4 ? written_header(block, chunk) : l.crcs[i];
    at[threadIdx.x] = (uint8_t)(word >> (8 * (threadIdx.x & 3u)));
  }
  strided_copy(at + kDataHeaderBytes, to_global(raw ? l.in_ptrs[i] : l.slots[i]), raw ? chunk : block,
               (uint64_t)blockIdx.y * kBlock + threadIdx.x, (uint64_t)gridDim.y * kBlock);
}

__global__ void write_end_kernel(const unsigned long long* cursor, size_t* frame_bytes) { *frame_bytes = (size_t)*cursor; }

__global__ void set_size_kernel(size_t* word, size_t value) { *word = value; }

// ---- reading: the walk ---------------------------------------------------------------------------------------
__global__ void read_reset_kernel(ReadState* st)
{
  ReadState z = {};
  *st = z;
}

// One lane: the chain is serial by the format's construction.  Between two calls the walk stands in front of a
// chunk or at the end of the input.  A pass ends in front of the data chunk that does not fit it any more, so what
// lies between and behind the data chunks (identifiers, padding) is passed with the chunks before it.
// lists: false counts only and goes to the end.
__device__ __forceinline__ void read_walk(const uint8_t* in_, uint64_t n, ReadState* stp, ReadLists l, bool lists,
                                          uint32_t capacity)
{
  cgptr in = to_global(in_);
  ReadState st = *stp;
  uint32_t count = 0;
  while (st.reason == kOk && !st.done) {
    if (st.pos == n) {
      st.done = 1;
      break;
    }
    Chunk c;
    const uint32_t r = parse_chunk(load_window(in, n, st.pos), n - st.pos, !st.started, c);
    if (r != kOk) {
      st.reason = r;
      break;
    }
    st.started = 1;
    if (c.kind != kSkipped) {
      if (lists && count == capacity)
        break;
      if (lists) {
        l.payloads[count] = in_ + st.pos + kDataHeaderBytes;
        l.batch_bytes[count] = c.kind == kCompressed ? c.payload : 0;
        l.content[count] = c.content;
        l.crcs[count] = c.crc;
        l.flags[count] = c.kind == kStored ? kEntryStored : 0;
      }
      count += 1;
      st.chunks += 1;
      st.content += c.content;
    }
    st.pos += c.bytes;
  }
  if (lists) {
    st.count = count;
    // (fewer chunks than the caller launches for: entries that ask nothing of anyone)
    for (uint32_t i = count; i < capacity; ++i) {
      l.payloads[i] = in_;
      l.batch_bytes[i] = 0;
      l.batch_caps[i] = 0;
      l.out_ptrs[i] = nullptr;
      l.content[i] = 0;
      l.crcs[i] = 0;
      l.flags[i] = kEntryStored | kEntryFailed;
    }
  }
  st.walked += count; // (the data chunks this call stepped over)
  *stp = st;
}

__global__ void read_walk_kernel(const uint8_t* in, uint64_t n, ReadState* stp, ReadLists l, bool lists, uint32_t capacity)
{
  read_walk(in, n, stp, l, lists, capacity);
}

// The walk behind the passes of an indexed read (snappy_frame_index_launch.hpp): where they listed and placed
// everything, *skip says so and nothing is left to do here.  (A kernel of its own: the walk of a stream without an
// index is the kernel above, without a word to load and test.)
__global__ void read_walk_unless_kernel(const uint8_t* in, uint64_t n, ReadState* stp, ReadLists l, bool lists,
                                        uint32_t capacity, const uint32_t* skip)
{
  if (*skip)
    return;
  read_walk(in, n, stp, l, lists, capacity);
}

// ---- reading: places -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanBlock) void read_scan_kernel(ReadLists l, ReadState* st, uint8_t* out, uint64_t out_bytes)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  const uint32_t count = st->count;
  uint64_t base = st->out_cursor;
  bool bad = false;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t i = tile + threadIdx.x;
    const uint64_t size = i < count ? l.content[i] : 0;
    uint64_t total;
    const uint64_t off = base + block_scan(size, lds, total);
    if (i < count) {
      const bool room = off <= out_bytes && size <= out_bytes - off;
      if (!room) { // the chunk gets no place: nothing of it is decoded or copied
        bad = true;
        l.flags[i] |= kEntryFailed;
        l.batch_bytes[i] = 0;
      }
      l.out_ptrs[i] = out + (off < out_bytes ? off : out_bytes);
      l.batch_caps[i] = room && !(l.flags[i] & kEntryStored) ? (size_t)size : 0;
    }
    base += total;
  }
  if (bad)
    atomicOr(&st->verdict, kVerdictCannotDecompress);
  __syncthreads();
  if (threadIdx.x == 0)
    st->out_cursor = base;
}

// ---- reading: the chunks -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void read_stored_kernel(ReadLists l, const ReadState* st)
{
  const uint32_t i = blockIdx.x;
  if (i >= st->count || (l.flags[i] & (kEntryStored | kEntryFailed)) != kEntryStored)
    return;
  strided_copy(to_global(l.out_ptrs[i]), to_global(l.payloads[i]), l.content[i], (uint64_t)blockIdx.y * kBlock + threadIdx.x,
               (uint64_t)gridDim.y * kBlock);
}

__global__ void read_verdict_kernel(ReadLists l, ReadState* st)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count || (l.flags[i] & (kEntryStored | kEntryFailed)))
    return;
  if (l.statuses[i] != hipcompSuccess || l.actual[i] != l.content[i]) {
    l.flags[i] |= kEntryFailed;
    atomicOr(&st->verdict, kVerdictCannotDecompress);
  }
}

// one wave per entry, grid-stride: the output's masked CRC-32C against the chunk's (a chunk whose decode failed
// has no output to speak of)
__global__ __launch_bounds__(kBlock) void read_crcs_kernel(ReadLists l, ReadState* st)
{
  __shared__ LdsTables L;
  fill_tables(L);
  const int lane = lane_id();
  const uint32_t count = st->count, waves = gridDim.x * kWavesPerBlock;
  for (uint32_t i = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; i < count; i += waves) {
    if (l.flags[i] & kEntryFailed)
      continue;
    const uint32_t crc = wave_crc(L, l.out_ptrs[i], l.content[i], lane);
    if (lane == 0 && mask_crc(crc) != l.crcs[i])
      atomicOr(&st->verdict, kVerdictBadChecksum);
  }
}

__global__ void read_finish_kernel(const ReadState* st, uint64_t num_chunks, uint64_t out_bytes, hipcompStatus_t* status)
{
  if (st->verdict & kVerdictBadChecksum)
    *status = hipcompErrorBadChecksum;
  else if (st->reason != kOk || (st->verdict & kVerdictCannotDecompress) || !st->done || st->chunks != num_chunks
           || st->out_cursor != out_bytes)
    *status = hipcompErrorCannotDecompress;
  else
    *status = hipcompSuccess;
}

inline uint32_t groups(uint64_t threads) { return (uint32_t)((threads + kBlock - 1) / kBlock); }
// workgroups of a CRC kernel for `count` chunks: enough to fill every CU (the LDS tables hold 9 per CU), few enough
// that each copies its tables for many chunks
inline uint32_t crc_groups(uint32_t count)
{
  const uint32_t want = (count + kWavesPerBlock - 1) / kWavesPerBlock, cap = (uint32_t)num_cus_of_current_device() * 8;
  return want < cap ? want : cap;
}
// workgroups per chunk of up to `bytes`: one per 16 KiB (a data chunk has 64 KiB at the most)
inline uint32_t parts_of(uint64_t bytes)
{
  const uint64_t p = (bytes + 16383) / 16384;
  return (uint32_t)(p < 1 ? 1 : p > 4 ? 4 : p);
}

} // namespace

hipError_t launch_write_begin(uint8_t* frame, unsigned long long* cursor, hipStream_t stream)
{
  write_begin_kernel<<<1, kWave, 0, stream>>>(frame, cursor);
  return hipGetLastError();
}

hipError_t launch_write_lists(const uint8_t* in, uint64_t in_size, uint64_t chunk_bytes, uint64_t first, uint32_t count,
                              uint8_t* slots, uint64_t slot_bytes, const WriteLists& l, hipStream_t stream)
{
  write_lists_kernel<<<groups(count), kBlock, 0, stream>>>(in, in_size, chunk_bytes, first, count, slots, slot_bytes, l);
  return hipGetLastError();
}

hipError_t launch_write_crcs(const WriteLists& l, uint32_t count, hipStream_t stream)
{
  write_crcs_kernel<<<crc_groups(count), kBlock, 0, stream>>>(l, count);
  return hipGetLastError();
}

hipError_t launch_write_scan(const WriteLists& l, uint32_t count, unsigned long long* cursor, hipStream_t stream)
{
  write_scan_kernel<<<1, kScanBlock, 0, stream>>>(l, count, cursor);
  return hipGetLastError();
}

hipError_t launch_write_chunks(uint8_t* frame, const WriteLists& l, uint32_t count, uint64_t chunk_bytes, hipStream_t stream)
{
  write_chunks_kernel<<<dim3(count, parts_of(chunk_bytes)), kBlock, 0, stream>>>(frame, l, count);
  return hipGetLastError();
}

hipError_t launch_write_end(const unsigned long long* cursor, size_t* frame_bytes, hipStream_t stream)
{
  write_end_kernel<<<1, 1, 0, stream>>>(cursor, frame_bytes);
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
                            hipStream_t stream, const uint32_t* skip)
{
  if (skip)
    read_walk_unless_kernel<<<1, 1, 0, stream>>>(in, in_bytes, st, lists ? *lists : ReadLists(), lists != nullptr, capacity,
                                                 skip);
  else
    read_walk_kernel<<<1, 1, 0, stream>>>(in, in_bytes, st, lists ? *lists : ReadLists(), lists != nullptr, capacity);
  return hipGetLastError();
}

hipError_t launch_read_scan(const ReadLists& l, ReadState* st, uint8_t* out, uint64_t out_bytes, hipStream_t stream)
{
  read_scan_kernel<<<1, kScanBlock, 0, stream>>>(l, st, out, out_bytes);
  return hipGetLastError();
}

hipError_t launch_read_stored(const ReadLists& l, const ReadState* st, uint32_t capacity, uint64_t largest_chunk,
                              hipStream_t stream)
{
  read_stored_kernel<<<dim3(capacity, parts_of(largest_chunk)), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_verdict(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream)
{
  read_verdict_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_crcs(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream)
{
  read_crcs_kernel<<<crc_groups(capacity), kBlock, 0, stream>>>(l, st);
  return hipGetLastError();
}

hipError_t launch_read_finish(const ReadState* st, uint64_t num_chunks, uint64_t out_bytes, hipcompStatus_t* status,
                              hipStream_t stream)
{
  read_finish_kernel<<<1, 1, 0, stream>>>(st, num_chunks, out_bytes, status);
  return hipGetLastError();
}

} // namespace szf
} // namespace hcamd
