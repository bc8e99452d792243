// lz4_frame_kernels.hip -- the kernels of the LZ4 manager's frame methods (lz4_frame_launch.hpp; the format and its
// arithmetic: lz4_frame.hpp, xxh32_math.hpp; the passes they make up: hlif.hip).
//
// Writing: the batched encoder fills a slot per chunk; a scan of the stored sizes continues from a cursor on the
// device, the block checksums are hashed, and the assembly kernel puts size word, bytes and checksum in place.
// Reading: one lane follows the block chain (each size word says where the next stands) and lists the blocks of a
// pass; sizes come from a parse, places from a scan; the batched decoder takes the compressed blocks of
// independent-block frames, a copy the stored ones, and a decoder that knows the frame's history -- one wave per
// frame, block after block -- those of linked-block frames.  Every store is a vector store.
#include "lz4_frame_launch.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace lz4f {

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;
constexpr int kWavesPerBlock = kBlock / kWave;

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

// XXH32 (seed 0) of len bytes at p by the four lanes of a quad: lane `sub` of it is accumulator `sub` and takes
// the dword at 4 * sub of every 16-byte stripe.  Every lane of the wave calls this (the accumulators change hands
// by a cross-lane read); all four lanes of a quad get the same p and len and return the hash.
__device__ __forceinline__ uint32_t quad_xxh32(cgptr p, uint64_t len, int lane)
{
  const int sub = lane & 3;
  uint32_t acc = xxh32::acc_init(sub, 0);
  const uint64_t stripes = len >> 4;
  cgptr q = p + 4 * sub;
  for (uint64_t s = 0; s < stripes; ++s, q += 16)
    acc = xxh32::round(acc, load_u32_any(q));
  const int quad = lane & ~3;
  const uint32_t v1 = (uint32_t)__shfl((int)acc, quad), v2 = (uint32_t)__shfl((int)acc, quad + 1),
                 v3 = (uint32_t)__shfl((int)acc, quad + 2), v4 = (uint32_t)__shfl((int)acc, quad + 3);
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

__device__ __forceinline__ uint32_t read32(const uint8_t* p)
{
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// exclusive scan over the kScanBlock threads of a workgroup; total: the sum
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

// One lane.  Between two calls the walk stands in front of a frame (or a skippable one, or the end of the input)
// or, in_frame, at the size word of a data block: a block is listed together with the look at what follows it, so
// the entry of a frame's last block says so (kLast) and its trailer is behind the walk.
// lists: false counts only and goes to the end.  final: the caller expects no more blocks; one that comes stops the
// walk short of the end.
__device__ __forceinline__ void read_walk(const uint8_t* in, uint64_t n, ReadState* stp, ReadLists l, bool lists,
                                          uint32_t capacity, bool final, bool verify)
{
  ReadState st = *stp;
  const uint64_t blocks_before = st.blocks;
  uint32_t count = 0;
  int32_t head = -1;
  while (st.reason == kOk && !st.done) {
    if (lists && !final && count == capacity)
      break;
    if (!st.in_frame) {
      if (st.pos == n) {
        st.done = 1;
        break;
      }
      if (n - st.pos < 4) {
        st.reason = kTruncated;
        break;
      }
      if (is_skippable(read32(in + st.pos))) {
        if (n - st.pos < 8 || read32(in + st.pos + 4) > n - st.pos - 8) {
          st.reason = kTruncated;
          break;
        }
        st.pos += 8 + (uint64_t)read32(in + st.pos + 4);
        continue;
      }
      Descriptor d;
      const uint32_t r = parse_descriptor(in + st.pos, n - st.pos, d);
      if (r != kOk) {
        st.reason = r;
        break;
      }
      st.pos += d.header_bytes;
      st.in_frame = 1;
      st.cur_flags = (d.linked ? kLinked : 0) | (d.block_checksums ? kBlockSum : 0) | (d.content_checksum ? kContentSum : 0);
      for (uint32_t code = 4; code <= 7; ++code)
        if (block_max_of_code(code) == d.block_max)
          st.cur_flags |= code << 8;
      st.cur_content = d.has_content_size ? d.content_size : kNoContentSize;
      st.frames += 1;
      if (d.has_content_size)
        st.declared_sum += d.content_size;
      else
        st.all_declared = 0;
      if (!d.block_checksums && !d.content_checksum)
        st.bare_frames += 1;
      head = (int32_t)count;
      // a frame without a data block
      if (n - st.pos >= 4 && (read32(in + st.pos) & ~kStoredBit) == 0) {
        st.pos += 4;
        if (st.cur_flags & kContentSum) {
          if (n - st.pos < 4) {
            st.reason = kTruncated;
            break;
          }
          if (verify && read32(in + st.pos) != xxh32::hash(nullptr, 0, 0))
            st.verdict |= kVerdictBadChecksum;
          st.pos += 4;
        }
        if (st.cur_content != kNoContentSize && st.cur_content != 0) {
          st.reason = kContentSize;
          break;
        }
        st.in_frame = 0;
      }
      continue;
    }
    if (n - st.pos < 4) {
      st.reason = kMissingEndMark;
      break;
    }
    const uint32_t word = read32(in + st.pos);
    const uint64_t size = word & ~kStoredBit;
    const uint32_t block_max = block_max_of_code((st.cur_flags >> 8) & 7u);
    if (size > block_max) {
      st.reason = kBlockTooLarge;
      break;
    }
    const uint64_t need = size + ((st.cur_flags & kBlockSum) ? 4 : 0);
    if (need > n - st.pos - 4) {
      st.reason = kTruncated;
      break;
    }
    if (st.blocks == 0xFFFFFFFFull) {
      st.reason = kTooManyBlocks;
      break;
    }
    if (lists && final)
      break; // (not done: launch_read_finish refuses)
    uint32_t flags = (st.cur_flags & ~kContentSum) | ((word & kStoredBit) ? kStored : 0);
    uint64_t aux = kNoContentSize;
    const uint8_t* const data = in + st.pos + 4;
    st.pos += 4 + need;
    st.blocks += 1;
    // what follows: the EndMark and the trailer, or the next block's size word (looked at again in its turn)
    if (n - st.pos >= 4 && (read32(in + st.pos) & ~kStoredBit) == 0) {
      st.pos += 4;
      if (st.cur_flags & kContentSum) {
        if (n - st.pos < 4) {
          st.reason = kTruncated;
          break;
        }
        st.pos += 4;
        flags |= kContentSum;
      }
      flags |= kLast;
      aux = st.cur_content;
      st.in_frame = 0;
    }
    if (lists) {
      l.comp_ptrs[count] = data;
      l.comp_bytes[count] = (size_t)size;
      l.batch_bytes[count] = (flags & (kStored | kLinked)) ? 0 : (size_t)size;
      l.flags[count] = flags;
      l.head[count] = head;
      l.aux[count] = aux;
    }
    count += 1;
  }
  if (lists) {
    st.count = count;
    // (fewer blocks than the caller launches for: entries that ask nothing of anyone)
    for (uint32_t i = count; i < capacity; ++i) {
      l.comp_ptrs[i] = in;
      l.comp_bytes[i] = 0;
      l.batch_bytes[i] = 0;
      l.batch_caps[i] = 0;
      l.out_ptrs[i] = nullptr;
      l.flags[i] = kStored;
      l.head[i] = -1;
      l.aux[i] = kNoContentSize;
    }
  }
  st.walked += (uint32_t)(st.blocks - blocks_before); // (the blocks this call stepped over)
  *stp = st;
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
// linear small-integer code at comp[c...) for one lane on its own: false where the stream ends inside it
__device__ __forceinline__ bool lane_read_length(const uint8_t* comp, uint32_t& c, uint32_t end, uint64_t& num)
{
  for (;;) {
    if (c >= end)
      return false;
    const uint32_t b = comp[c];
    ++c;
    num += b;
    if (b != 255u)
      return true;
  }
}

// The decoded size of a compressed block of a linked frame: the token walk alone, one lane per block (the sizes do
// not depend on the history; whether the offsets are sound the decoder says).  A stream that does not parse: 0.
// (The loop has one exit, `ok` or the end of the stream, on purpose: a first form that left it by `break` from
// several places gave a block a wrong size when the lane beside it was done earlier -- seen on the MI355X with two
// blocks of unlike length codes, not explained from the source; tests/test_lz4_frame_gpu.py, linked_long_runs.)
__global__ void read_linked_sizes_kernel(ReadLists l, const ReadState* st)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count)
    return;
  const uint32_t flags = l.flags[i];
  if (!(flags & kLinked) || (flags & kStored))
    return;
  const uint8_t* const comp = l.comp_ptrs[i];
  const uint32_t end = (uint32_t)l.comp_bytes[i]; // (at most the block maximum, 4 MiB)
  uint64_t d = 0;
  uint32_t c = 0;
  bool ok = true;
  while (ok && c < end) {
    const uint32_t tok = comp[c];
    ++c;
    uint64_t lit = tok >> 4;
    if (lit == 15)
      ok = lane_read_length(comp, c, end, lit);
    if (!ok || lit > end - c) {
      ok = false;
      continue;
    }
    c += (uint32_t)lit;
    d += lit;
    if (c >= end)
      continue; // the last sequence: literals only
    if (end - c < 2) {
      ok = false;
      continue;
    }
    c += 2;
    uint64_t ml = 4 + (tok & 15u);
    if ((tok & 15u) == 15)
      ok = lane_read_length(comp, c, end, ml);
    d += ml;
  }
  l.sizes[i] = ok ? (size_t)d : 0;
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

// linear small-integer code at comp[c...): false where the stream ends inside it
__device__ __forceinline__ bool read_length(cgptr comp, uint32_t& c, uint32_t end, uint32_t& num)
{
  for (;;) {
    if (c >= end)
      return false;
    const uint32_t b = uniform((uint32_t)comp[c]);
    ++c;
    num += b; // (end <= 4 MiB: below 2^31)
    if (b != 255u)
      return true;
  }
}

// One block of a linked frame by one wave: the token walk is wave-uniform (scalar), literal runs and matches are
// copied across the lanes.  The history is what the frame has produced: out[frame_start, at), written by this
// wave just now, by the stored-block copy before this kernel or by earlier passes.  `at`: where the block's output
// starts, cap: its parsed size.  An offset may reach back to frame_start and no further.
__device__ bool decode_linked_block(cgptr comp, uint32_t end, gptr out, uint64_t frame_start, uint64_t at, uint32_t cap,
                                    int lane)
{
  uint32_t c = 0, d = 0;
  while (c < end) {
    const uint32_t tok = uniform((uint32_t)comp[c]);
    ++c;
    uint32_t lit = tok >> 4;
    if (lit == 15 && !read_length(comp, c, end, lit))
      return false;
    if (lit > cap - d || lit > end - c)
      return false;
    if (lit <= (uint32_t)kWave) {
      if ((uint32_t)lane < lit)
        out[at + d + lane] = comp[c + lane];
    } else {
      wave_copy(out + at + d, comp + c, lit, lane);
    }
    c += lit;
    d += lit;
    if (c >= end)
      break;
    if (end - c < 2)
      return false;
    const uint32_t offset = uniform((uint32_t)comp[c] | ((uint32_t)comp[c + 1] << 8));
    c += 2;
    uint32_t ml = 4 + (tok & 15u);
    if ((tok & 15u) == 15 && !read_length(comp, c, end, ml))
      return false;
    if (offset == 0 || (uint64_t)offset > at + d - frame_start || ml > cap - d)
      return false;
    // (stores of this wave to out[] are ordered before its later loads: one wave, in-order vector memory)
    gptr dst = out + at + d;
    cgptr src = dst - offset;
    if (offset >= ml) {
      if (ml <= (uint32_t)kWave) {
        if ((uint32_t)lane < ml)
          dst[lane] = src[lane];
      } else {
        wave_copy(dst, src, ml, lane);
      }
    } else if ((offset & (offset - 1u)) == 0) {
      for (uint32_t i = (uint32_t)lane; i < ml; i += kWave)
        dst[i] = src[i & (offset - 1u)];
    } else {
      for (uint32_t i = (uint32_t)lane; i < ml; i += kWave)
        dst[i] = src[i % offset];
    }
    d += ml;
  }
  return d == cap;
}

// Wave w of the grid: if entry w is the first one of a linked frame in this pass, the wave decodes that frame's
// blocks of the pass one after the other; every other wave leaves.
__global__ __launch_bounds__(kBlock) void read_linked_kernel(ReadLists l, ReadState* st, uint8_t* out_base)
{
  const uint32_t w = blockIdx.x * kWavesPerBlock + uniform((uint32_t)(threadIdx.x >> 6));
  const uint32_t count = st->count;
  if (w >= count || !(l.flags[w] & kLinked))
    return;
  const int32_t head = l.head[w];
  if (!(head == (int32_t)w || (head < 0 && w == 0)))
    return;
  const int lane = lane_id();
  gptr out = to_global(out_base);
  const uint64_t frame_start = head >= 0 ? (uint64_t)(l.out_ptrs[w] - out_base) : st->frame_out_start;
  for (uint32_t e = w; e < count; ++e) {
    const uint32_t flags = uniform(l.flags[e]);
    if (e > w && (int32_t)uniform((uint32_t)l.head[e]) != head)
      break;
    if (!(flags & kStored)) {
      const uint32_t cap = uniform((uint32_t)l.caps[e]);
      const uint64_t at = uniform((uint64_t)(l.out_ptrs[e] - out_base));
      const bool ok = decode_linked_block(to_global(uniform_ptr(l.comp_ptrs[e])), uniform((uint32_t)l.comp_bytes[e]), out,
                                          frame_start, at, cap, lane);
      if (!ok) {
        if (lane == 0)
          atomicOr(&st->verdict, kVerdictCannotDecompress);
        return; // (what follows in this frame would read what was not written)
      }
    }
    if (flags & kLast)
      break;
  }
}

__global__ void read_verdict_kernel(ReadLists l, ReadState* st)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= st->count || (l.flags[i] & (kStored | kLinked)))
    return;
  if (l.statuses[i] != hipcompSuccess || l.actual[i] != l.caps[i])
    atomicOr(&st->verdict, kVerdictCannotDecompress);
}

// a quad per block: the XXH32 of the block's bytes in the frame against the four bytes behind them
__global__ void read_block_sums_kernel(ReadLists l, ReadState* st)
{
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x, i = t >> 2;
  const bool on = i < st->count && (l.flags[i] & kBlockSum);
  const uint8_t* const p = on ? l.comp_ptrs[i] : nullptr;
  const uint64_t n = on ? l.comp_bytes[i] : 0;
  const uint32_t h = quad_xxh32(to_global(p), n, lane_id());
  if (on && (t & 3) == 0 && h != read32(p + n))
    atomicOr(&st->verdict, kVerdictBadChecksum);
}

// Wave w: if entry w ends a frame with a content checksum, the first quad of the wave hashes the frame's content
// -- one chain of stripes by the construction of the hash -- and compares.  (Runs behind the pass's decoders.)
__global__ __launch_bounds__(kBlock) void read_content_sums_kernel(ReadLists l, ReadState* st, uint8_t* out)
{
  const uint32_t w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (w >= st->count)
    return;
  const uint32_t flags = l.flags[w];
  if ((flags & (kLast | kContentSum)) != (kLast | kContentSum))
    return;
  // (a frame whose decode failed has no content to speak of: the refusal stands, as LZ4F_decompress's does)
  if (st->verdict & kVerdictCannotDecompress)
    return;
  const int32_t head = l.head[w];
  const uint64_t start = head >= 0 ? (uint64_t)(l.out_ptrs[head] - out) : st->frame_out_start;
  const uint64_t end = (uint64_t)(l.out_ptrs[w] - out) + l.caps[w];
  const int lane = lane_id();
  const uint32_t h = quad_xxh32(to_global(out + start), lane < 4 ? end - start : 0, lane);
  const uint8_t* const sum = l.comp_ptrs[w] + l.comp_bytes[w] + ((flags & kBlockSum) ? 4 : 0) + 4;
  if (lane == 0 && h != read32(sum))
    atomicOr(&st->verdict, kVerdictBadChecksum);
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

inline uint32_t groups(uint64_t threads) { return (uint32_t)((threads + kBlock - 1) / kBlock); }
// workgroups per block of up to `bytes`: one per 32 KiB, up to 128
inline uint32_t parts_of(uint64_t bytes)
{
  const uint64_t p = bytes / 32768;
  return (uint32_t)(p < 1 ? 1 : p > 128 ? 128 : p);
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
