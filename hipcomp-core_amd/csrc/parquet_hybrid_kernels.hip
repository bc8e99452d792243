// parquet_hybrid_kernels.hip -- the kernel of a decode of a batch of Parquet RLE / bit-packed hybrid streams in one
// call (parquet_hybrid_launch.hpp; the arithmetic and the rules: parquet_hybrid_plan.hpp).
//
// An item is a stream: a chain of runs, each a ULEB128 header and either one value (an RLE run) or groups of 8
// bit-packed values.  One wavefront per item follows the chain (walk_runs of the plan, the very code the host tests
// run) twice: first without storing, so that an item the rules refuse -- wherever in it the damage lies -- has no
// byte of its output written; then to decode.
//
// The chain is serial and wave-uniform: all 64 lanes run the parser on the same state.  The header bytes come
// through a register window: 64 bytes of the stream in one coalesced load, lane l keeping byte l, every byte the
// parser asks for read from the window's lane with a uniform index (v_readlane), the window loaded anew where the
// parser leaves it; the bytes of a bit-packed run are stepped over by arithmetic.  The values of a run are parallel:
// lane l takes value base + l of it, 64 at a time.  No LDS.  Every store is a vector store.
#include "parquet_hybrid_launch.hpp"

#include "byte_window.hpp"
#include "device_facts.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace pqh {

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

// the element in every place of a dword
template <class T>
__device__ __forceinline__ uint32_t spread(T v)
{
  return sizeof(T) == 1 ? (uint32_t)v * 0x01010101u : sizeof(T) == 2 ? (uint32_t)v * 0x00010001u : (uint32_t)v;
}

// What the decoding walk does with a run: all lanes, values [first, first + count) of the item's output.
template <class T>
struct WaveSink
{
  typedef HC_GLOBAL T* optr;
  cgptr p;    // the item
  uint64_t n; // its bytes
  optr out;
  uint32_t match;
  int lane;
  uint64_t rle_matches = 0; // wave-uniform
  uint64_t mine = 0;        // this lane's matches in bit-packed runs

  // `count` copies of one value: elements up to the first dword boundary, dwords, the elements behind the last
  // whole dword.  Nothing outside the count elements is written.
  __device__ __forceinline__ void rle(uint64_t first, uint64_t count, uint32_t value)
  {
    const T v = (T)value;
    if ((uint32_t)v == match)
      rle_matches += count;
    const optr d = out + first;
    uint64_t head = ((0 - (uint64_t)reinterpret_cast<uintptr_t>(d)) & 3u) / sizeof(T); // (d lies at T's alignment)
    head = head < count ? head : count;
    if ((uint64_t)lane < head)
      d[lane] = v;
    const uint64_t dwords = (count - head) * sizeof(T) / 4;
    HC_GLOBAL uint32_t* const body = reinterpret_cast<HC_GLOBAL uint32_t*>(d + head);
    const uint32_t word = spread(v);
    for (uint64_t i = (uint64_t)lane; i < dwords; i += kWave)
      body[i] = word;
    const uint64_t done = head + dwords * (4 / sizeof(T));
    if ((uint64_t)lane < count - done)
      d[done + lane] = v;
  }

  // Lane l takes value k0 + l, k0 = 0, 64, ...: k0 values are k0 / 8 * bit_width whole bytes, the lane's place
  // behind them is the plan's where_of.  The 8 bytes at the value's first byte in two dword loads where the item
  // has them, else the value's own bytes one by one: nothing outside the item is read.
  __device__ __forceinline__ void packed(uint64_t first, uint64_t count, uint64_t data, uint32_t bit_width)
  {
    const Where w = where_of((uint64_t)lane, bit_width);
    for (uint64_t k0 = 0; k0 < count; k0 += kWave) {
      const uint64_t k = k0 + (uint64_t)lane;
      if (k < count) {
        const uint64_t at = data + (k0 >> 3) * bit_width + w.byte;
        uint64_t bytes8 = 0;
        if (at + 8 <= n) {
          bytes8 = (uint64_t)load_u32_any(p + at) | ((uint64_t)load_u32_any(p + at + 4) << 32);
        } else {
          for (uint32_t j = 0; j < w.bytes; ++j)
            bytes8 |= (uint64_t)p[at + j] << (8 * j);
        }
        const T v = (T)value_of(bytes8, w.shift, bit_width);
        out[first + k] = v;
        mine += (uint32_t)v == match ? 1u : 0u;
      }
    }
  }

  // once per item
  __device__ __forceinline__ uint64_t matches() const
  {
    const uint64_t sum = wave_scan_add_u64(mine);
    return rle_matches + ((uint64_t)read_lane((uint32_t)sum, kWave - 1) | ((uint64_t)read_lane((uint32_t)(sum >> 32), kWave - 1) << 32));
  }
};

// wave w of the grid takes items w, w + waves, ...: all its lanes, on the same state
template <class T>
__global__ __launch_bounds__(kBlock) void decode_kernel(Batch b)
{
  const int lane = lane_id();
  for (uint64_t it = (uint64_t)blockIdx.x * kWavesPerBlock + uniform((uint32_t)(threadIdx.x >> 6)); it < b.items;
       it += (uint64_t)gridDim.x * kWavesPerBlock) {
    const uint8_t* const p = uniform_ptr(b.stream_ptrs[it]);
    const uint64_t n = uniform((uint64_t)b.stream_bytes[it]);
    const uint32_t bit_width = b.form == kWidthPrefixed ? 0u : uniform(b.bit_widths[it]);
    const uint64_t wanted = uniform((uint64_t)b.num_values[it]);
    const uint64_t capacity = uniform((uint64_t)b.out_capacities[it]);
    WindowSrc src(to_global(p), n, lane);
    const Frame f = frame_of(src, n, b.form, bit_width, wanted, capacity, (uint32_t)(8 * sizeof(T)));
    Walk w;
    uint64_t matches = 0;
    if (f.ok) {
      NoSink none;
      w = walk_runs(src, f.pos, f.end, f.bit_width, wanted, none);
      if (w.ok) {
        WaveSink<T> sink;
        sink.p = to_global(p);
        sink.n = n;
        sink.out = (typename WaveSink<T>::optr)uniform_ptr(b.out_ptrs[it]);
        sink.match = b.match_values ? uniform(b.match_values[it]) : 0u;
        sink.lane = lane;
        w = walk_runs(src, f.pos, f.end, f.bit_width, wanted, sink);
        if (b.match_counts)
          matches = sink.matches();
      }
    }
    const Verdict v = verdict_of(f, w, b.form);
    if (lane == 0) {
      b.statuses[it] = v.ok ? hipcompSuccess : hipcompErrorCannotDecompress;
      if (b.consumed_bytes)
        b.consumed_bytes[it] = (size_t)v.consumed;
      if (b.match_counts)
        b.match_counts[it] = v.ok ? (size_t)matches : 0;
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

template <class T>
hipError_t launch_as(const Batch& b, hipStream_t stream)
{
  decode_kernel<T><<<walk_groups((const void*)decode_kernel<T>, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

} // namespace

hipError_t launch(const Batch& b, uint32_t element_bytes, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  switch (element_bytes) {
  case 1: return launch_as<uint8_t>(b, stream);
  case 2: return launch_as<uint16_t>(b, stream);
  case 4: return launch_as<uint32_t>(b, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace pqh
} // namespace hcamd
