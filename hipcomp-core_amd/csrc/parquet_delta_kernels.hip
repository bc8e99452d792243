// parquet_delta_kernels.hip -- the kernel of a decode of a batch of Parquet DELTA_BINARY_PACKED streams in one call
// (parquet_delta_launch.hpp; the arithmetic and the rules: parquet_delta_plan.hpp).
//
// An item is a stream: a header of four varints, then blocks, each a minimum delta, a width byte per miniblock and the
// miniblocks' bit-packed deltas.  One wavefront per item follows the blocks (walk_blocks of the plan, the very code the
// host tests run) twice: first without storing, so that an item the rules refuse -- wherever in it the damage lies --
// has no byte of its output written; then to decode.
//
// The parse is serial and wave-uniform: all 64 lanes run it on the same state, the header bytes, minimum deltas and
// width bytes coming through the register window (byte_window.hpp).  A step of the walk is 64 consecutive values of a
// block, whatever the miniblock size: lane l unpacks delta l of the step from its own miniblock -- one of the two the
// step touches --, adds the minimum delta, and a prefix sum over the wave plus the carry of the step before gives the
// values.  Under Offsets a second prefix sum, over the lengths and carried in 64 bits, gives the offsets.  No LDS.
// Every store is a vector store, an element per lane.
#include "parquet_delta_launch.hpp"

#include <type_traits>

#include "byte_window.hpp"
#include "device_facts.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace pqd {

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
static_assert(kStep == (uint32_t)kWave, "a step of the plan's walk is a wavefront's lanes");

__device__ __forceinline__ uint32_t last_lane(uint32_t v) { return read_lane(v, kWave - 1); }
__device__ __forceinline__ uint64_t last_lane(uint64_t v)
{
  return (uint64_t)read_lane((uint32_t)v, kWave - 1) | ((uint64_t)read_lane((uint32_t)(v >> 32), kWave - 1) << 32);
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) { return wave_scan_add_u32(v); }
__device__ __forceinline__ uint64_t wave_scan_add(uint64_t v) { return wave_scan_add_u64(v); }

// Packed delta k of the miniblock at `data` of the item p[0, n), of `width` bits: at most 32 (kBits 32: the 8 bytes at
// the value's first byte) or 64 (kBits 64: 9 of the 12).  Dword loads where the item has the bytes, else the value's
// own bytes one by one: nothing outside the item is read.
template <uint32_t kBits>
__device__ __forceinline__ uint64_t unpack(cgptr p, uint64_t n, uint64_t data, uint32_t k, uint32_t width)
{
  const Where w = where_of((uint64_t)k, width);
  const uint64_t at = data + w.byte;
  uint64_t lo = 0;
  uint32_t hi = 0;
  if (width == 0)
    return 0;
  if (at + (kBits > 32 ? 12 : 8) <= n) {
    lo = (uint64_t)load_u32_any(p + at) | ((uint64_t)load_u32_any(p + at + 4) << 32);
    if (kBits > 32)
      hi = load_u32_any(p + at + 8);
  } else {
    for (uint32_t j = 0; j < w.bytes; ++j) {
      const uint32_t b = (uint32_t)p[at + j];
      if (j < 8)
        lo |= (uint64_t)b << (8 * j);
      else
        hi = b;
    }
  }
  return kBits > 32 ? value_of64(lo, hi, w.shift, width) : (uint64_t)pqh::value_of(lo, w.shift, width);
}

// What a walk does with a step: all lanes.  T: the elements; kLengths: the stream holds lengths (Offsets), the elements
// are their running sums; kStore: the decoding walk (the first walk under Offsets is this without the stores: it has
// to see every length and their sum).  `last`, `sum` and `negative` are wave-uniform.
template <class T, bool kLengths, bool kStore>
struct WaveSink
{
  typedef HC_GLOBAL T* optr;
  typedef typename std::conditional<kLengths, uint32_t, T>::type D; // the delta layer
  cgptr p;    // the item
  uint64_t n; // its bytes
  optr out;
  int lane;
  D last;           // the value before the step
  uint64_t sum = 0; // of the lengths so far

  // value 0, the header's: a length under Offsets
  __device__ __forceinline__ bool begin(uint64_t total)
  {
    bool ok = true;
    if (kLengths) {
      if (kStore && lane == 0)
        out[0] = 0;
      if (total) {
        ok = !negative_length((uint32_t)last);
        sum = (uint64_t)last;
        if (kStore && lane == 0)
          out[1] = (T)sum;
      }
    } else if (kStore && total && lane == 0) {
      out[0] = (T)last;
    }
    return ok;
  }

  __device__ __forceinline__ bool step(uint64_t first, uint32_t count, uint64_t min_delta, const Piece& a, uint32_t k0, uint32_t split,
                                       const Piece& b)
  {
    const uint32_t l = (uint32_t)lane;
    const bool active = l < count, in_a = l < split;
    D x = 0; // (0 in the lanes behind the step's values: lane 63 has the step's last value)
    if (active)
      x = (D)((D)min_delta + (D)unpack<8 * sizeof(T)>(p, n, in_a ? a.data : b.data, in_a ? k0 + l : l - split, in_a ? a.width : b.width));
    const D v = (D)(last + wave_scan_add(x));
    last = last_lane(v);
    if (!kLengths) {
      if (kStore && active)
        out[first + l] = (T)v;
      return true;
    }
    const bool negative = wave_ballot(active && negative_length((uint32_t)v)) != 0;
    const uint64_t offset = sum + wave_scan_add_u64(active ? (uint64_t)v : 0);
    sum = last_lane(offset);
    if (kStore && active)
      out[first + l + 1] = (T)offset;
    return !negative;
  }
};

// wave w of the grid takes items w, w + waves, ...: all its lanes, on the same state
template <class T, bool kLengths>
__global__ __launch_bounds__(kBlock) void decode_kernel(Batch b)
{
  typedef typename WaveSink<T, kLengths, true>::D D;
  constexpr uint32_t bits = (uint32_t)(8 * sizeof(T));
  const int lane = lane_id();
  for (uint64_t it = (uint64_t)blockIdx.x * kWavesPerBlock + uniform((uint32_t)(threadIdx.x >> 6)); it < b.items;
       it += (uint64_t)gridDim.x * kWavesPerBlock) {
    const uint8_t* const p = uniform_ptr(b.stream_ptrs[it]);
    const uint64_t n = uniform((uint64_t)b.stream_bytes[it]);
    const uint64_t wanted = b.num_values ? uniform((uint64_t)b.num_values[it]) : 0;
    const uint64_t capacity = uniform((uint64_t)b.out_capacities[it]);
    WindowSrc src(to_global(p), n, lane);
    const Header h = parse_header(src, n);
    Walk w;
    bool ok = fits(h, b.num_values != nullptr, wanted, capacity, kLengths ? kOffsets : kValues);
    if (ok) {
      if (kLengths) {
        WaveSink<T, kLengths, false> dry;
        dry.p = to_global(p);
        dry.n = n;
        dry.out = nullptr;
        dry.lane = lane;
        dry.last = (D)h.first;
        ok = dry.begin(h.total);
        if (ok) {
          w = walk_blocks(src, h, n, bits, dry);
          ok = w.ok && offsets_fit(dry.sum, n, w.pos, bits);
        }
      } else {
        NoSink none;
        w = walk_blocks(src, h, n, bits, none);
        ok = w.ok;
      }
    }
    if (ok) {
      WaveSink<T, kLengths, true> sink;
      sink.p = to_global(p);
      sink.n = n;
      sink.out = (typename WaveSink<T, kLengths, true>::optr)uniform_ptr(b.out_ptrs[it]);
      sink.lane = lane;
      sink.last = (D)h.first;
      (void)sink.begin(h.total);
      w = walk_blocks(src, h, n, bits, sink);
    }
    const Verdict v = verdict_of(ok, h, w);
    if (lane == 0) {
      b.statuses[it] = v.ok ? hipcompSuccess : hipcompErrorCannotDecompress;
      if (b.value_counts)
        b.value_counts[it] = (size_t)v.count;
      if (b.consumed_bytes)
        b.consumed_bytes[it] = (size_t)v.consumed;
    }
  }
}

// workgroups of a walk over num_items items: a wave each, no more than the device holds at once
uint32_t walk_groups(const void* kernel, uint64_t num_items)
{
  const uint64_t want = (num_items + kWavesPerBlock - 1) / kWavesPerBlock;
  const int per_cu = resident_per_cu(kernel, kBlock, 0);
  const uint64_t most = (uint64_t)num_cus_of_current_device() * (uint64_t)(per_cu > 0 ? per_cu : 1);
  return (uint32_t)(want < most ? want : most);
}

template <class T, bool kLengths>
hipError_t launch_as(const Batch& b, hipStream_t stream)
{
  decode_kernel<T, kLengths><<<walk_groups((const void*)decode_kernel<T, kLengths>, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

} // namespace

hipError_t launch(const Batch& b, uint32_t element_bytes, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  if (b.output != kValues && b.output != kOffsets)
    return hipErrorInvalidValue;
  const bool offsets = b.output == kOffsets;
  switch (element_bytes) {
  case 4: return offsets ? launch_as<uint32_t, true>(b, stream) : launch_as<uint32_t, false>(b, stream);
  case 8: return offsets ? launch_as<uint64_t, true>(b, stream) : launch_as<uint64_t, false>(b, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace pqd
} // namespace hcamd
