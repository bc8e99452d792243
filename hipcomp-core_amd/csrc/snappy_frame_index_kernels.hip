// snappy_frame_index_kernels.hip -- the kernels of seekable Snappy framed streams (snappy_frame_index_launch.hpp; the
// index and the tests it has to pass: snappy_frame_index.hpp; the passes: hlif.hip).
//
// Writing: the identifier and the fields, the words of every pass (the four bytes write_chunks_kernel puts in front
// of every data chunk, from the same lists) and, once they all stand, the CRC.  Reading: one workgroup hops from unit
// to unit -- per unit one lane reads the identifier and the fields and steps over what lies between the units, the
// workgroup sums the chunk lengths and computes the CRC -- and one workgroup per pass scans the lengths from a
// cursor on the device, gathers the 16 bytes at every scanned offset and writes the entries the chain's walk would
// have written.  The index is untrusted: every address is tested against the input's length before it is read.
// Every store is a vector store.
#include "snappy_frame_device.hiph"
#include "snappy_frame_index_launch.hpp"

namespace hcamd {
namespace szf {

namespace {

// The CRC-32C of a body of up to 16 MiB is cut into pieces of 64 KiB, what wave_crc takes and crc32c_shift reaches.
constexpr uint32_t kPieceBytes = 65536;
constexpr uint32_t kMaxPieces = (32 + 4 * kIndexMaxChunks + kPieceBytes - 1) / kPieceBytes; // 257

struct CrcLds
{
  LdsTables tables;
  uint32_t piece[kMaxPieces + 1];
};

// CRC-32C of p[0, bytes), bytes <= 32 + 4 * kIndexMaxChunks, by the kScanBlock threads of a workgroup (tables
// filled), the result in every thread: one wave per piece, then one lane joins the pieces in their order --
// crc(A || B) = crc(A) * x^(8|B|) ^ crc(B), every shift below 2^17 bytes.
__device__ uint32_t group_crc(CrcLds& c, const uint8_t* p, uint64_t bytes)
{
  const uint32_t pieces = (uint32_t)((bytes + kPieceBytes - 1) / kPieceBytes);
  const int lane = lane_id();
  for (uint32_t k = threadIdx.x / kWave; k < pieces; k += kScanBlock / kWave) {
    const uint64_t at = (uint64_t)k * kPieceBytes;
    const uint32_t len = bytes - at < kPieceBytes ? (uint32_t)(bytes - at) : kPieceBytes;
    const uint32_t crc = wave_crc(c.tables, p + at, len, lane);
    if (lane == 0)
      c.piece[k] = crc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t crc = 0;
    for (uint32_t k = 0; k < pieces; ++k) {
      const uint64_t at = (uint64_t)k * kPieceBytes;
      const uint32_t len = bytes - at < kPieceBytes ? (uint32_t)(bytes - at) : kPieceBytes;
      crc = crc32c::crc32c_shift(c.tables.x2n, crc, len) ^ c.piece[k];
    }
    c.piece[kMaxPieces] = crc;
  }
  __syncthreads();
  const uint32_t crc = c.piece[kMaxPieces];
  __syncthreads();
  return crc;
}

// ---- writing -------------------------------------------------------------------------------------------------
__global__ void index_write_begin_kernel(uint8_t* frame, unsigned long long* cursor, uint32_t chunks, uint32_t chunk_bytes,
                                         uint64_t content_bytes)
{
  uint8_t h[kIndexWordsAt];
  write_index_fields(h, chunks, chunk_bytes, content_bytes);
  for (uint32_t k = 0; k < kIdentifierBytes; ++k)
    frame[k] = (uint8_t)identifier().byte(k);
  for (uint32_t k = 0; k < kIndexWordsAt; ++k)
    frame[kIdentifierBytes + k] = h[k];
  *cursor = kIdentifierBytes + index_bytes(chunks);
}

__global__ void index_write_words_kernel(uint8_t* index, WriteLists l, uint64_t first, uint32_t count)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count)
    return;
  store_u32_any(to_global(index) + kIndexWordsAt + 4 * (first + i), written_header(l.block_bytes[i], l.in_bytes[i]));
}

__global__ __launch_bounds__(kScanBlock) void index_write_end_kernel(uint8_t* index, uint32_t chunks)
{
  __shared__ CrcLds c;
  fill_tables(c.tables);
  const uint64_t body = 32 + 4 * (uint64_t)chunks;
  const uint32_t crc = group_crc(c, index + 4, body);
  if (threadIdx.x == 0)
    store_u32_any(to_global(index) + 4 + body, mask_crc(crc));
}

// ---- reading: from unit to unit ------------------------------------------------------------------------------
struct Hop // what one lane finds where a unit begins, and behind it, for the workgroup
{
  uint32_t reason;
  uint32_t stop; // a refusal, or the end of the input behind the unit: no further unit to work on
  IndexedEntry e;
  uint64_t index_at;
};

__global__ __launch_bounds__(kScanBlock) void index_begin_kernel(const uint8_t* in, uint64_t n, IndexState* ix)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  __shared__ Hop hop;
  __shared__ CrcLds c;
  fill_tables(c.tables);
  cgptr gin = to_global(in);
  uint64_t pos = 0, chunks = 0, content = 0;
  uint32_t units = 0, reason = kIndexOk;
  for (;;) {
    // pos: where an identifier is due
    if (threadIdx.x == 0) {
      IndexHead h;
      Chunk id;
      uint32_t r = kIndexOk;
      if (n - pos < kIdentifierBytes || in[pos] != kTypeIdentifier || parse_chunk(load_window(gin, n, pos), n - pos, false, id) != kOk)
        r = kIndexNotThere;
      const uint64_t index_at = pos + kIdentifierBytes;
      if (r == kIndexOk)
        r = parse_index_fields(in + index_at, n - index_at, h);
      if (r == kIndexOk && (units == kMaxIndexedStreams || chunks + h.chunks > 0xFFFFFFFFull))
        r = kIndexTooManyUnits;
      hop.reason = r;
      hop.stop = r != kIndexOk;
      if (r == kIndexOk) {
        hop.index_at = index_at;
        hop.e.words_at = index_at + kIndexWordsAt;
        hop.e.data_at = index_at + index_bytes(h.chunks);
        hop.e.first_chunk = chunks;
        hop.e.out_start = content;
        hop.e.content_bytes = h.content_bytes;
        hop.e.chunks = h.chunks;
        hop.e.chunk_bytes = h.chunk_bytes;
      }
    }
    __syncthreads();
    if (hop.stop) {
      reason = hop.reason;
      break;
    }
    const IndexedEntry e = hop.e;
    const uint64_t index_at = hop.index_at;
    // the bytes of the data chunks: the words lie inside the input (parse_index_fields: the chunk's length does)
    uint64_t v = 0;
    for (uint64_t i = threadIdx.x; i < e.chunks; i += kScanBlock)
      v += indexed_chunk_bytes(load_u32_any(gin + e.words_at + 4 * i));
    uint64_t total;
    block_scan(v, lds, total);
    const uint64_t body = 32 + 4 * (uint64_t)e.chunks;
    const uint32_t crc = group_crc(c, in + index_at + 4, body);
    // (every thread comes to the same verdict)
    const uint64_t end_at = e.data_at + total;
    if (mask_crc(crc) != load_u32_any(gin + index_at + 4 + body))
      reason = kIndexCrc;
    else if (end_at > n)
      reason = kIndexOffset;
    if (reason != kIndexOk)
      break;
    // what stands behind the sum: one lane steps over padding and skippable chunks
    if (threadIdx.x == 0) {
      uint64_t next = end_at;
      bool more = false;
      hop.reason = step_behind_unit(in, n, next, more);
      hop.stop = hop.reason != kIndexOk || !more;
      hop.index_at = next;
      ix->unit[units] = e;
    }
    __syncthreads();
    units += 1;
    chunks += e.chunks;
    content += e.content_bytes;
    reason = hop.reason;
    pos = hop.index_at;
    const bool stop = hop.stop;
    __syncthreads(); // (hop is written again)
    if (stop)
      break;
  }
  if (threadIdx.x == 0) {
    ix->ok = reason == kIndexOk;
    ix->reason = reason;
    ix->skip = 0;
    ix->units = units;
    ix->chunks = chunks;
    ix->content_bytes = content;
    ix->listed = 0;
    ix->cursor = 0;
    ix->cur = 0;
    ix->reserved = 0;
  }
}

// ---- reading: the entries of a pass --------------------------------------------------------------------------
// entries that ask nothing of anyone: the walk's for a pass with fewer chunks than the caller launches for
__device__ __forceinline__ void ask_nothing(const ReadLists& l, const uint8_t* in, uint32_t capacity)
{
  for (uint32_t i = threadIdx.x; i < capacity; i += blockDim.x) {
    l.payloads[i] = in;
    l.batch_bytes[i] = 0;
    l.batch_caps[i] = 0;
    l.out_ptrs[i] = nullptr;
    l.content[i] = 0;
    l.crcs[i] = 0;
    l.flags[i] = kEntryStored | kEntryFailed;
  }
}

__global__ __launch_bounds__(kScanBlock) void index_list_kernel(const uint8_t* in, uint64_t n, IndexState* ix, ReadState* st,
                                                                ReadLists l, bool lists, uint32_t capacity)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  __shared__ uint32_t refused;
  if (threadIdx.x == 0)
    refused = kIndexOk;
  __syncthreads();
  if (!ix->ok) {
    if (lists)
      ask_nothing(l, in, capacity);
    if (threadIdx.x == 0)
      st->count = 0;
    return;
  }
  const uint64_t before = ix->listed, all = ix->chunks;
  // (a caller that asks for more chunks than the units hold: not this path's business, the chain's reader says so)
  const uint64_t want = lists ? (uint64_t)capacity : all - before;
  uint32_t cur = ix->cur;
  uint64_t cursor = ix->cursor, listed = 0;
  uint32_t why = all - before < want ? (uint32_t)kIndexCount : (uint32_t)kIndexOk;
  cgptr gin = to_global(in);
  while (why == kIndexOk && listed < want) {
    const IndexedEntry f = ix->unit[cur];
    const uint64_t b0 = before + listed - f.first_chunk; // the unit's first chunk of this pass
    const uint64_t left = f.chunks - b0, room = want - listed;
    const uint64_t take = left < room ? left : room;
    uint64_t base = b0 == 0 ? f.data_at : cursor;
    for (uint64_t tile = 0; tile < take; tile += kScanBlock) {
      const uint64_t i = tile + threadIdx.x, b = b0 + i;
      const bool on = i < take;
      const uint32_t word = on ? load_u32_any(gin + f.words_at + 4 * b) : 0;
      const uint64_t bytes = on ? indexed_chunk_bytes(word) : 0;
      uint64_t total;
      const uint64_t off = base + block_scan(bytes, lds, total);
      if (on) {
        const uint32_t share = b + 1 < f.chunks ? f.chunk_bytes : (uint32_t)(f.content_bytes - (uint64_t)f.chunk_bytes * b);
        uint32_t r = kIndexOk;
        Window w;
        // the whole chunk inside the input: its header, and with a type of 0x00 / 0x01 and the length that fits it
        // its CRC and the first payload byte
        if (off > n || n - off < bytes)
          r = kIndexOffset;
        else {
          w = load_window(gin, n, off);
          r = check_indexed_chunk(word, w.word(0), w, share);
        }
        if (r == kIndexOk && lists) {
          const uint64_t e = listed + i;
          const bool raw = (word & 0xFFu) == kTypeStored;
          l.payloads[e] = in + off + kDataHeaderBytes;
          l.batch_bytes[e] = raw ? 0 : (size_t)((word >> 8) - 4);
          l.content[e] = share;
          l.crcs[e] = w.word(4);
          l.flags[e] = raw ? kEntryStored : 0;
        }
        if (r != kIndexOk)
          atomicMax(&refused, r);
      }
      base += total;
    }
    cursor = base;
    listed += take;
    if (b0 + take == f.chunks)
      cur += 1;
    __syncthreads();
    why = refused;
  }
  __syncthreads();
  if (why == kIndexOk)
    why = refused;
  if (why != kIndexOk) {
    if (lists)
      ask_nothing(l, in, capacity);
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
  if (i >= st->count || (l.flags[i] & kEntryStored))
    return;
  // (a chunk read_scan_kernel gave no place: the configuration is another input's, the chain's reader says so)
  if ((l.flags[i] & kEntryFailed) || l.statuses[i] != hipcompSuccess || l.actual[i] != l.content[i]) {
    ix->reason = kIndexDecode;
    ix->ok = 0;
  }
}

__global__ void index_end_kernel(IndexState* ix, ReadState* st, ReadLists l, uint32_t capacity, const uint8_t* in, uint64_t n,
                                 uint64_t num_chunks)
{
  // (ok, listed and chunks are not written here: every thread reads the same)
  const bool held = ix->ok && ix->listed == ix->chunks && ix->chunks == num_chunks;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (held && i < capacity) {
    l.payloads[i] = in;
    l.batch_bytes[i] = 0;
    l.batch_caps[i] = 0;
    l.out_ptrs[i] = nullptr;
    l.content[i] = 0;
    l.crcs[i] = 0;
    l.flags[i] = kEntryStored | kEntryFailed;
  }
  if (i != 0)
    return;
  ix->skip = held;
  if (held) {
    st->pos = n;
    st->chunks = ix->chunks;
    st->content = ix->content_bytes;
    st->started = 1;
    st->done = 1;
    st->count = 0;
  } else {
    ReadState z = {};
    *st = z;
  }
}

// ---- ranged reads ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanBlock) void index_range_list_kernel(const uint8_t* in, uint64_t n, const IndexState* ix,
                                                                      uint32_t unit, range::Plan plan, uint64_t pass_first,
                                                                      uint32_t count, uint8_t* out, RangeSlots slots, ReadLists l,
                                                                      size_t* caps, ReadState* st)
{
  __shared__ uint64_t lds[kScanBlock / kWave + 1];
  const IndexedEntry f = ix->unit[unit];
  cgptr gin = to_global(in);
  // where chunk pass_first stands: behind the chunks before it
  uint64_t v = 0, total;
  for (uint64_t b = threadIdx.x; b < pass_first; b += kScanBlock)
    v += indexed_chunk_bytes(load_u32_any(gin + f.words_at + 4 * b));
  block_scan(v, lds, total);
  uint64_t base = f.data_at + total;
  bool bad = false;
  for (uint32_t tile = 0; tile < count; tile += kScanBlock) {
    const uint32_t i = tile + threadIdx.x;
    const bool on = i < count;
    const uint64_t b = pass_first + i;
    const uint32_t word = on ? load_u32_any(gin + f.words_at + 4 * b) : 0;
    const uint64_t bytes = on ? indexed_chunk_bytes(word) : 0;
    const uint64_t off = base + block_scan(bytes, lds, total);
    if (on) {
      const range::Span s = range::range_span(plan, b, pass_first);
      // (launch_index_list has tested every chunk of this input in its place: a chunk that does not pass now is
      // another input's, and asks nothing)
      bool inside = off <= n && n - off >= bytes;
      Window w;
      if (inside) {
        w = load_window(gin, n, off);
        inside = check_indexed_chunk(word, w.word(0), w, (uint32_t)s.cap) == kIndexOk;
      }
      const bool raw = (word & 0xFFu) == kTypeStored;
      bad = bad || !inside;
      l.payloads[i] = inside ? in + off + kDataHeaderBytes : in;
      l.batch_bytes[i] = inside && !raw ? (size_t)((word >> 8) - 4) : 0;
      l.out_ptrs[i] = s.edge ? slots.base + (uint64_t)s.slot * slots.stride : out + s.dst_at;
      l.batch_caps[i] = inside && !raw ? (size_t)s.cap : 0;
      l.content[i] = inside ? (uint32_t)s.cap : 0;
      l.crcs[i] = inside ? w.word(4) : 0;
      l.flags[i] = inside ? (raw ? kEntryStored : 0u) : kEntryStored | kEntryFailed;
      caps[i] = (size_t)s.cap;
    }
    base += total;
  }
  if (bad)
    atomicOr(&st->verdict, kVerdictCannotDecompress);
  if (threadIdx.x == 0)
    st->count = count;
}

__global__ void index_range_settle_kernel(ReadLists l, const size_t* caps, const ReadState* st)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count || !(l.flags[i] & kEntryStored))
    return;
  const bool failed = l.flags[i] & kEntryFailed;
  l.statuses[i] = failed ? hipcompErrorCannotDecompress : hipcompSuccess;
  l.actual[i] = failed ? 0 : caps[i];
}

__global__ void index_range_finish_kernel(const ReadState* st, hipcompStatus_t* status)
{
  if (st->verdict & kVerdictBadChecksum)
    *status = hipcompErrorBadChecksum;
  else if (st->verdict & kVerdictCannotDecompress)
    *status = hipcompErrorCannotDecompress;
  else
    *status = hipcompSuccess;
}

inline uint32_t groups(uint64_t threads) { return (uint32_t)((threads + kBlock - 1) / kBlock); }

} // namespace

hipError_t launch_index_write_begin(uint8_t* frame, unsigned long long* cursor, uint32_t chunks, uint32_t chunk_bytes,
                                    uint64_t content_bytes, hipStream_t stream)
{
  index_write_begin_kernel<<<1, 1, 0, stream>>>(frame, cursor, chunks, chunk_bytes, content_bytes);
  return hipGetLastError();
}

hipError_t launch_index_write_words(uint8_t* index, const WriteLists& l, uint64_t first, uint32_t count, hipStream_t stream)
{
  index_write_words_kernel<<<groups(count), kBlock, 0, stream>>>(index, l, first, count);
  return hipGetLastError();
}

hipError_t launch_index_write_end(uint8_t* index, uint32_t chunks, hipStream_t stream)
{
  index_write_end_kernel<<<1, kScanBlock, 0, stream>>>(index, chunks);
  return hipGetLastError();
}

hipError_t launch_index_begin(const uint8_t* in, uint64_t in_bytes, IndexState* ix, hipStream_t stream)
{
  index_begin_kernel<<<1, kScanBlock, 0, stream>>>(in, in_bytes, ix);
  return hipGetLastError();
}

hipError_t launch_index_list(const uint8_t* in, uint64_t in_bytes, IndexState* ix, ReadState* st, const ReadLists* lists,
                             uint32_t capacity, hipStream_t stream)
{
  index_list_kernel<<<1, kScanBlock, 0, stream>>>(in, in_bytes, ix, st, lists ? *lists : ReadLists(), lists != nullptr, capacity);
  return hipGetLastError();
}

hipError_t launch_index_verdict(const ReadLists& l, const ReadState* st, IndexState* ix, uint32_t capacity, hipStream_t stream)
{
  index_verdict_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, st, ix);
  return hipGetLastError();
}

hipError_t launch_index_end(IndexState* ix, ReadState* st, const ReadLists& l, uint32_t capacity, const uint8_t* in,
                            uint64_t in_bytes, uint64_t num_chunks, hipStream_t stream)
{
  index_end_kernel<<<groups(capacity ? capacity : 1), kBlock, 0, stream>>>(ix, st, l, capacity, in, in_bytes, num_chunks);
  return hipGetLastError();
}

hipError_t launch_index_range_list(const uint8_t* in, uint64_t in_bytes, const IndexState* ix, uint32_t unit,
                                   const range::Plan& plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                                   const RangeSlots& slots, const ReadLists& l, size_t* caps, ReadState* st, hipStream_t stream)
{
  index_range_list_kernel<<<1, kScanBlock, 0, stream>>>(in, in_bytes, ix, unit, plan, pass_first, count, out, slots, l, caps, st);
  return hipGetLastError();
}

hipError_t launch_index_range_settle(const ReadLists& l, const size_t* caps, const ReadState* st, uint32_t capacity,
                                     hipStream_t stream)
{
  index_range_settle_kernel<<<groups(capacity), kBlock, 0, stream>>>(l, caps, st);
  return hipGetLastError();
}

hipError_t launch_index_range_finish(const ReadState* st, hipcompStatus_t* status, hipStream_t stream)
{
  index_range_finish_kernel<<<1, 1, 0, stream>>>(st, status);
  return hipGetLastError();
}

} // namespace szf
} // namespace hcamd
