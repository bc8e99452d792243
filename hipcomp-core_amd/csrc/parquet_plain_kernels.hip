// parquet_plain_kernels.hip -- the kernels of the three calls that put a Parquet page's dense values into their rows, the
// nulls placed (parquet_plain_launch.hpp; the arithmetic and the rules: parquet_plain_plan.hpp).
//
// One wavefront per item, the waves of the grid striding over the items.  Every item is walked twice: first without
// storing, so that an item the rules refuse -- wherever in it the damage lies -- has no byte of its outputs written;
// then to write.  (A dense item of fixed-width values or booleans has nothing to walk the first time: its rules are
// all about its counts.)
//
// The rows go in steps of 64, lane l row l of the step: a ballot of the valid rows is 8 bytes of the validity bitmap,
// the count of the valid lanes below plus the wave-uniform carry of the steps before is the lane's place among the
// values, so consecutive valid lanes read consecutive values.  Values of 4 and 8 bytes are one unaligned load (or,
// byte-stream-split, 4 or 8 byte loads, each coalesced across the lanes) and one coalesced store per lane; other widths
// are cut into units of 4 bytes (or of 1 where the width is no multiple of 4) that the lanes take in order, each finding
// its row's place in the row's lane (ds_bpermute: the crossbar, no LDS memory).  Booleans: a second ballot, of the
// valid rows whose bit is set, is the step's 8 bytes of the values bitmap.  Strings: a 64-bit wave scan of the lengths
// sums the first walk's total, a 32-bit one gives the second walk's 64 offsets; packed bytes are one stretch of the body
// once the offsets are proven to rise, copied 16 bytes a lane; length-prefixed bytes are taken by the lanes in order,
// each finding its row by a binary search among the step's 64 inclusive sums.  No LDS, no scratch.  Every store is a
// vector store.
#include "parquet_plain_launch.hpp"

#include "device_facts.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace pqv {

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
static_assert(kStep == (uint32_t)kWave, "a step of the rows is a wavefront's lanes");

template <class U>
__device__ __forceinline__ U load_any(cgptr p)
{
  typedef U __attribute__((aligned(1))) unaligned;
  return *reinterpret_cast<const HC_GLOBAL unaligned*>(p);
}
// the unit of a byte-stream-split value: byte b of it lies `stride` bytes behind byte b - 1
template <class U>
__device__ __forceinline__ U load_split(cgptr p, uint64_t stride)
{
  U v = 0;
#pragma unroll
  for (uint32_t b = 0; b < sizeof(U); ++b)
    v |= (U)((U)p[(uint64_t)b * stride] << (8 * b));
  return v;
}
__device__ __forceinline__ uint32_t last_lane(uint32_t v) { return read_lane(v, kWave - 1); }
__device__ __forceinline__ uint64_t last_lane(uint64_t v)
{
  return (uint64_t)read_lane((uint32_t)v, kWave - 1) | ((uint64_t)read_lane((uint32_t)(v >> 32), kWave - 1) << 32);
}
// the value lane `from` holds (from < 64, any per lane); every lane of the wave has to be here
__device__ __forceinline__ uint32_t from_lane(uint32_t v, uint32_t from)
{
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(from << 2), (int)v);
}
__device__ __forceinline__ uint64_t from_lane(uint64_t v, uint32_t from)
{
  return (uint64_t)from_lane((uint32_t)v, from) | ((uint64_t)from_lane((uint32_t)(v >> 32), from) << 32);
}
// the set bits of a ballot in the lanes below this one
__device__ __forceinline__ uint32_t lanes_set_below(uint64_t mask)
{
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint64_t first_item() { return (uint64_t)blockIdx.x * kWavesPerBlock + uniform((uint32_t)(threadIdx.x >> 6)); }
__device__ __forceinline__ uint64_t item_stride() { return (uint64_t)gridDim.x * kWavesPerBlock; }

// ---- the rows of an item ---------------------------------------------------------------------------------------------------
// A step: rows [base, base + 64), lane l row base + l.  `carry` is wave-uniform.
struct PlaceWalk
{
  cgptr levels; // nullptr: dense
  uint64_t rows;
  uint32_t max_level;
  uint64_t num_values;
  uint64_t src_bytes, start; // of the item's source
  int lane;
  uint64_t carry = 0; // the valid rows before the step
  // of the step:
  uint64_t mask = 0;  // the valid rows
  bool valid = false; // this lane's row
  bool have = false;  // and its value is there: always, once the item is accepted
  uint32_t below = 0; // the valid rows of the step below this lane: the row's value is carry-before-the-step + below
  uint64_t at = 0;

  __device__ __forceinline__ void load(const PlaceBatch& b, uint64_t it, int lane_)
  {
    lane = lane_;
    num_values = uniform((uint64_t)b.num_values[it]);
    levels = b.level_ptrs ? to_global(uniform_ptr(b.level_ptrs[it])) : nullptr;
    rows = b.level_ptrs ? uniform((uint64_t)b.num_rows[it]) : num_values;
    max_level = b.level_ptrs ? uniform(b.max_levels[it]) : 0u;
    src_bytes = uniform((uint64_t)b.src_bytes[it]);
    start = b.value_starts ? uniform((uint64_t)b.value_starts[it]) : 0;
  }
  // false: a level of the step refuses the item (wave-uniform)
  __device__ __forceinline__ bool step(uint64_t base)
  {
    const uint64_t r = base + (uint64_t)lane;
    const bool active = r < rows;
    uint32_t level = max_level;
    if (levels && active)
      level = (uint32_t)levels[r];
    valid = active && level_valid(level, max_level);
    mask = wave_ballot(valid);
    below = lanes_set_below(mask);
    at = carry + below;
    have = valid && at < num_values;
    carry += (uint64_t)__builtin_popcountll(mask);
    return wave_ballot(active && level_refused(level, max_level)) == 0;
  }
  // the first walk of an item whose rules beyond the counts are the levels' alone
  __device__ __forceinline__ bool levels_accepted()
  {
    bool ok = true;
    if (levels) {
      for (uint64_t base = 0; ok && base < rows; base += kStep)
        ok = step(base);
      ok = ok && carry == num_values;
      carry = 0;
    }
    return ok;
  }
  // after the last step of a first walk
  __device__ __forceinline__ bool counted() const { return !levels || carry == num_values; }
  // 8 bytes of a bitmap of the rows, by 8 lanes
  __device__ __forceinline__ void store_bits(gptr bitmap, uint64_t base, uint64_t bits) const
  {
    const uint64_t byte = (base >> 3) + (uint64_t)lane;
    if (lane < 8 && byte < bitmap_bytes(rows))
      bitmap[byte] = (uint8_t)(bits >> (8 * lane));
  }
};

// ---- place_parquet_values ---------------------------------------------------------------------------------------------
// U: the unit of a store; kOne: a value is one unit (4 and 8 bytes), else value_bytes / sizeof(U) of them; kSplit:
// kByteStreamSplit
template <class U, bool kOne, bool kSplit>
__global__ __launch_bounds__(kBlock) void place_values_kernel(PlaceBatch b)
{
  const int lane = lane_id();
  const uint32_t units = kOne ? 1u : b.value_bytes / (uint32_t)sizeof(U);
  for (uint64_t it = first_item(); it < b.items; it += item_stride()) {
    PlaceWalk w;
    w.load(b, it, lane);
    const Shape s = shape_of(b.level_ptrs != nullptr, w.num_values, w.rows, uniform((uint64_t)b.out_capacities[it]), 0);
    bool ok = s.ok && !start_refused(w.start, w.src_bytes) && values_fit(w.num_values, b.value_bytes, w.src_bytes - w.start);
    ok = ok && w.levels_accepted();
    if (ok) {
      const cgptr src = to_global(uniform_ptr(b.src_ptrs[it])) + w.start;
      HC_GLOBAL U* const out = (HC_GLOBAL U*)uniform_ptr(b.out_ptrs[it]);
      const gptr validity = b.validity_ptrs ? to_global(uniform_ptr(b.validity_ptrs[it])) : nullptr;
      for (uint64_t base = 0; base < w.rows; base += kStep) {
        const uint64_t before = w.carry;
        (void)w.step(base);
        if (kOne) {
          if (base + (uint64_t)lane < w.rows) {
            U v = 0;
            if (w.have)
              v = kSplit ? load_split<U>(src + w.at, w.num_values) : load_any<U>(src + w.at * sizeof(U));
            out[base + (uint64_t)lane] = v;
          }
        } else {
          const uint64_t left = w.rows - base;
          const uint32_t step_units = (uint32_t)(left < kStep ? left : kStep) * units;
          for (uint32_t t = 0; t < step_units; t += kStep) {
            const uint32_t j = t + (uint32_t)lane;
            const uint32_t q = j / units;
            const uint32_t row = q < kStep ? q : kStep - 1;
            const uint64_t place = before + from_lane(w.below, row);
            const uint32_t u = j - row * units; // the unit of the value
            const bool valid = (w.mask >> row) & 1;
            if (j < step_units) {
              U v = 0;
              if (valid)
                v = kSplit ? load_split<U>(src + (uint64_t)u * sizeof(U) * w.num_values + place, w.num_values)
                           : load_any<U>(src + (place * units + u) * sizeof(U));
              out[base * units + j] = v;
            }
          }
        }
        if (validity)
          w.store_bits(validity, base, w.mask);
      }
    }
    if (lane == 0)
      b.statuses[it] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
  }
}

// ---- place_parquet_booleans ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void place_booleans_kernel(PlaceBatch b)
{
  const int lane = lane_id();
  for (uint64_t it = first_item(); it < b.items; it += item_stride()) {
    PlaceWalk w;
    w.load(b, it, lane);
    const Shape s = shape_of(b.level_ptrs != nullptr, w.num_values, w.rows, uniform((uint64_t)b.out_capacities[it]), 0);
    bool ok = s.ok && !start_refused(w.start, w.src_bytes) && bits_fit(w.num_values, w.src_bytes - w.start);
    ok = ok && w.levels_accepted();
    if (ok) {
      const cgptr src = to_global(uniform_ptr(b.src_ptrs[it])) + w.start;
      const gptr out = to_global((uint8_t*)uniform_ptr(b.out_ptrs[it]));
      const gptr validity = b.validity_ptrs ? to_global(uniform_ptr(b.validity_ptrs[it])) : nullptr;
      for (uint64_t base = 0; base < w.rows; base += kStep) {
        (void)w.step(base);
        bool set = false;
        if (w.have)
          set = ((uint32_t)src[w.at >> 3] >> (uint32_t)(w.at & 7)) & 1u;
        w.store_bits(out, base, wave_ballot(set));
        if (validity)
          w.store_bits(validity, base, w.mask);
      }
    }
    if (lane == 0)
      b.statuses[it] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
  }
}

// ---- place_parquet_strings -----------------------------------------------------------------------------------------------
template <bool kIsPacked>
__global__ __launch_bounds__(kBlock) void place_strings_kernel(PlaceBatch b)
{
  constexpr uint32_t layout = kIsPacked ? kPacked : kLengthPrefixed;
  const int lane = lane_id();
  for (uint64_t it = first_item(); it < b.items; it += item_stride()) {
    PlaceWalk w;
    w.load(b, it, lane);
    const HC_GLOBAL int32_t* const off = (const HC_GLOBAL int32_t*)uniform_ptr(b.value_offsets[it]);
    const uint64_t byte_capacity = uniform((uint64_t)b.byte_capacities[it]);
    const Shape s = shape_of(b.level_ptrs != nullptr, w.num_values, w.rows, uniform((uint64_t)b.offset_capacities[it]), 1);
    bool ok = s.ok && !start_refused(w.start, w.src_bytes);
    const uint64_t behind = ok ? w.src_bytes - w.start : 0;
    uint64_t total = 0; // wave-uniform
    // the first walk reads levels and offsets, no byte of the body
    for (uint64_t base = 0; ok && base < w.rows; base += kStep) {
      ok = w.step(base);
      if (ok) {
        int32_t from = 0, to = 0;
        if (w.have) {
          from = off[w.at];
          to = off[w.at + 1];
        }
        const bool refused = w.have && string_refused(layout, w.at, from, to, behind);
        const uint64_t sums = wave_scan_add_u64(refused ? 0 : (uint64_t)(uint32_t)(to - from));
        total += last_lane(sums);
        ok = wave_ballot(refused) == 0 && !total_refused(total, byte_capacity);
      }
    }
    ok = ok && w.counted();
    if (ok) {
      const cgptr body = to_global(uniform_ptr(b.src_ptrs[it])) + w.start;
      HC_GLOBAL int32_t* const out = (HC_GLOBAL int32_t*)uniform_ptr(b.out_offsets[it]);
      const gptr bytes = to_global(uniform_ptr(b.out_bytes[it]));
      const gptr validity = b.validity_ptrs ? to_global(uniform_ptr(b.validity_ptrs[it])) : nullptr;
      uint32_t written = 0; // the bytes before the step: at most 2^31 - 1
      w.carry = 0;
      if (lane == 0)
        out[0] = 0;
      for (uint64_t base = 0; base < w.rows; base += kStep) {
        (void)w.step(base);
        uint32_t length = 0;
        uint64_t source = 0; // where the row's bytes lie in the body
        if (w.have) {
          const int32_t from = off[w.at];
          length = (uint32_t)(off[w.at + 1] - from);
          source = string_at(layout, w.at, (uint64_t)from);
        }
        const uint32_t ends = wave_scan_add_u32(length); // the row's end among the step's bytes
        const uint32_t step_bytes = last_lane(ends);
        if (base + (uint64_t)lane < w.rows)
          out[base + (uint64_t)lane + 1] = (int32_t)(written + ends);
        if (!kIsPacked) {
          const uint32_t begins = ends - length;
          // (a step of empty or null rows: no byte)
          for (uint32_t t = 0; t < step_bytes; t += kStep) {
            const uint32_t j = t + (uint32_t)lane;
            uint32_t row = 0; // the first row that ends behind byte j
            for (uint32_t half = kStep / 2; half; half >>= 1)
              if (from_lane(ends, row + half - 1) <= j)
                row += half;
            const uint32_t begin = from_lane(begins, row);
            const uint64_t src = from_lane(source, row);
            if (j < step_bytes)
              bytes[(uint64_t)written + j] = body[src + (j - begin)];
          }
        }
        written += step_bytes;
        if (validity)
          w.store_bits(validity, base, w.mask);
      }
      // the offsets rise from off[0] to off[num_values] inside the body: the values' bytes are that one stretch
      if (kIsPacked && total != 0)
        wave_copy(bytes, body + (uint64_t)uniform((uint32_t)off[0]), (uint32_t)total, lane);
    }
    if (lane == 0) {
      b.statuses[it] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
      if (b.out_byte_counts)
        b.out_byte_counts[it] = ok ? (size_t)total : 0;
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

template <class U, bool kOne, bool kSplit>
hipError_t place_as(const PlaceBatch& b, hipStream_t stream)
{
  place_values_kernel<U, kOne, kSplit><<<walk_groups((const void*)place_values_kernel<U, kOne, kSplit>, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}
template <bool kSplit>
hipError_t place_by_width(const PlaceBatch& b, hipStream_t stream)
{
  if (b.value_bytes == 8)
    return place_as<uint64_t, true, kSplit>(b, stream);
  if (b.value_bytes == 4)
    return place_as<uint32_t, true, kSplit>(b, stream);
  return b.value_bytes % 4 == 0 ? place_as<uint32_t, false, kSplit>(b, stream) : place_as<uint8_t, false, kSplit>(b, stream);
}

} // namespace

hipError_t launch_place_values(const PlaceBatch& b, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  if (b.value_bytes < 1 || b.value_bytes > kMaxValueBytes || !value_layout_known(b.layout))
    return hipErrorInvalidValue;
  return b.layout == kByteStreamSplit ? place_by_width<true>(b, stream) : place_by_width<false>(b, stream);
}

hipError_t launch_place_booleans(const PlaceBatch& b, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  place_booleans_kernel<<<walk_groups((const void*)place_booleans_kernel, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

hipError_t launch_place_strings(const PlaceBatch& b, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  if (!string_layout_known(b.layout))
    return hipErrorInvalidValue;
  if (b.layout == kPacked)
    place_strings_kernel<true><<<walk_groups((const void*)place_strings_kernel<true>, b.items), kBlock, 0, stream>>>(b);
  else
    place_strings_kernel<false><<<walk_groups((const void*)place_strings_kernel<false>, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

} // namespace pqv
} // namespace hcamd
