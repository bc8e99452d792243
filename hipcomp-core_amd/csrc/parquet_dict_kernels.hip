// parquet_dict_kernels.hip -- the kernels of the three calls that gather a Parquet dictionary's entries to rows
// (parquet_dict_launch.hpp; the arithmetic and the rules: parquet_dict_plan.hpp).
//
// One wavefront per item, the waves of the grid striding over the items.  Every item is walked twice: first without
// storing, so that an item the rules refuse -- wherever in it the damage lies -- has no byte of its outputs written;
// then to write.
//
// index_kernel follows the chain of a BYTE_ARRAY dictionary page (walk_chain of the plan, the very code the host tests
// run): serial and wave-uniform, the length words coming through the register window (byte_window.hpp); lane k & 63
// keeps offset k + 1, and every 64 entries the wave stores its 64 offsets at once.
//
// The gathers take the rows in steps of 64, lane l row l of the step: a ballot of the valid rows is 8 bytes of the
// bitmap, the count of the valid lanes below plus the wave-uniform carry of the steps before is the lane's place among
// the indices.  Entries of 4 and 8 bytes are an unaligned load and a coalesced store per lane; other widths are cut
// into units of 4 bytes (or of 1 where the width is no multiple of 4) that the lanes take in order, each finding its
// row's index in the row's lane (ds_bpermute: the crossbar, no LDS memory).  Strings: a wave scan of the lengths gives
// the step's 64 offsets; the step's bytes are taken by the lanes in order, each finding its row by a binary search
// among the 64 inclusive sums.  No LDS, no scratch.  Every store is a vector store.
#include "parquet_dict_launch.hpp"

#include "byte_window.hpp"
#include "device_facts.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace pqg {

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
static_assert(kStep == (uint32_t)kWave, "a step of the gathers is a wavefront's lanes");

template <class U>
__device__ __forceinline__ U load_any(cgptr p)
{
  typedef U __attribute__((aligned(1))) unaligned;
  return *reinterpret_cast<const HC_GLOBAL unaligned*>(p);
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

// ---- index_parquet_dictionary -----------------------------------------------------------------------------------------
// the storing walk's sink: all lanes; k is wave-uniform
struct LaneSink
{
  HC_GLOBAL int32_t* out;
  int lane;
  int32_t mine = 0;
  __device__ __forceinline__ void take(uint64_t k, uint64_t off)
  {
    if (lane == (int)(k & 63))
      mine = (int32_t)off;
    if ((k & 63) == 63)
      out[k - 63 + 1 + (uint64_t)lane] = mine;
  }
  // the offsets of the last, partial 64
  __device__ __forceinline__ void finish(uint64_t entries)
  {
    if ((uint64_t)lane < (entries & 63))
      out[(entries & ~uint64_t(63)) + 1 + (uint64_t)lane] = mine;
  }
};

__global__ __launch_bounds__(kBlock) void index_kernel(IndexBatch b)
{
  const int lane = lane_id();
  for (uint64_t it = first_item(); it < b.items; it += item_stride()) {
    const uint8_t* const p = uniform_ptr(b.dict_ptrs[it]);
    const uint64_t n = uniform((uint64_t)b.dict_bytes[it]);
    const uint64_t entries = uniform((uint64_t)b.num_entries[it]);
    const uint64_t capacity = uniform((uint64_t)b.offset_capacities[it]);
    WindowSrc src(to_global(p), n, lane);
    NoSink none;
    const bool ok = offsets_fit(entries, capacity) && walk_chain(src, n, entries, none);
    if (ok) {
      LaneSink sink;
      sink.out = (HC_GLOBAL int32_t*)uniform_ptr(b.offset_ptrs[it]);
      sink.lane = lane;
      if (lane == 0)
        sink.out[0] = 0;
      (void)walk_chain(src, n, entries, sink);
      sink.finish(entries);
    }
    if (lane == 0) {
      b.statuses[it] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
      if (b.entry_counts)
        b.entry_counts[it] = ok ? (size_t)entries : 0;
    }
  }
}

// ---- the rows of a gathering item ---------------------------------------------------------------------------------------
// A step: rows [base, base + 64), lane l row base + l.  `carry` is wave-uniform.
struct RowWalk
{
  const HC_GLOBAL uint32_t* indices;
  uint64_t num_indices;
  cgptr levels; // nullptr: dense
  uint64_t rows;
  uint32_t max_level;
  uint64_t entries;
  int lane;
  uint64_t carry = 0; // the valid rows before the step
  // of the step:
  uint64_t mask = 0;  // the valid rows
  bool valid = false; // this lane's row
  bool indexed = false; // and its index is there and inside the dictionary
  uint32_t index = 0;

  __device__ __forceinline__ void load(const GatherBatch& b, uint64_t it, int lane_)
  {
    lane = lane_;
    indices = (const HC_GLOBAL uint32_t*)uniform_ptr(b.index_ptrs[it]);
    num_indices = uniform((uint64_t)b.num_indices[it]);
    levels = b.level_ptrs ? to_global(uniform_ptr(b.level_ptrs[it])) : nullptr;
    rows = b.level_ptrs ? uniform((uint64_t)b.num_rows[it]) : num_indices;
    max_level = b.level_ptrs ? uniform(b.max_levels[it]) : 0u;
    entries = uniform((uint64_t)b.dict_entries[it]);
  }
  // false: a level or an index of the step refuses the item (wave-uniform)
  __device__ __forceinline__ bool step(uint64_t base)
  {
    const uint64_t r = base + (uint64_t)lane;
    const bool active = r < rows;
    uint32_t level = max_level;
    if (levels && active)
      level = (uint32_t)levels[r];
    valid = active && level_valid(level, max_level);
    mask = wave_ballot(valid);
    const uint64_t at = carry + lanes_set_below(mask);
    const bool have = valid && at < num_indices;
    index = have ? indices[at] : 0u;
    indexed = have && !index_refused(index, entries);
    carry += (uint64_t)__builtin_popcountll(mask);
    return wave_ballot((active && level_refused(level, max_level)) || (have && !indexed)) == 0;
  }
  // after the last step of the first walk
  __device__ __forceinline__ bool counted() const { return !levels || carry == num_indices; }
  // 8 bytes of the bitmap, by 8 lanes
  __device__ __forceinline__ void store_validity(gptr validity, uint64_t base) const
  {
    const uint64_t byte = (base >> 3) + (uint64_t)lane;
    if (lane < 8 && byte < bitmap_bytes(rows))
      validity[byte] = (uint8_t)(mask >> (8 * lane));
  }
};

// ---- gather_parquet_dictionary ---------------------------------------------------------------------------------------
// U: the unit of a store; kOne: an entry is one unit (4 and 8 bytes), else entry_bytes / sizeof(U) of them
template <class U, bool kOne>
__global__ __launch_bounds__(kBlock) void gather_kernel(GatherBatch b)
{
  const int lane = lane_id();
  const uint32_t units = kOne ? 1u : b.entry_bytes / (uint32_t)sizeof(U);
  for (uint64_t it = first_item(); it < b.items; it += item_stride()) {
    RowWalk w;
    w.load(b, it, lane);
    const cgptr dict = to_global(uniform_ptr(b.dict_ptrs[it]));
    const uint64_t dict_bytes = uniform((uint64_t)b.dict_bytes[it]);
    const Shape s = shape_of(b.level_ptrs != nullptr, w.num_indices, w.rows, uniform((uint64_t)b.out_capacities[it]), 0);
    bool ok = s.ok && dictionary_fits(w.entries, dict_bytes, b.entry_bytes);
    for (uint64_t base = 0; ok && base < w.rows; base += kStep)
      ok = w.step(base);
    ok = ok && w.counted();
    if (ok) {
      HC_GLOBAL U* const out = (HC_GLOBAL U*)uniform_ptr(b.out_ptrs[it]);
      const gptr validity = b.validity_ptrs ? to_global(uniform_ptr(b.validity_ptrs[it])) : nullptr;
      w.carry = 0;
      for (uint64_t base = 0; base < w.rows; base += kStep) {
        (void)w.step(base);
        if (kOne) {
          if (base + (uint64_t)lane < w.rows)
            out[base + (uint64_t)lane] = w.valid ? load_any<U>(dict + (uint64_t)w.index * sizeof(U)) : (U)0;
        } else {
          const uint64_t left = w.rows - base;
          const uint32_t step_units = (uint32_t)(left < kStep ? left : kStep) * units;
          for (uint32_t t = 0; t < step_units; t += kStep) {
            const uint32_t j = t + (uint32_t)lane;
            const uint32_t q = j / units;
            const uint32_t row = q < kStep ? q : kStep - 1;
            const uint32_t index = from_lane(w.index, row);
            const bool valid = (w.mask >> row) & 1;
            if (j < step_units)
              out[base * units + j] = valid ? load_any<U>(dict + ((uint64_t)index * units + (j - row * units)) * sizeof(U)) : (U)0;
          }
        }
        if (validity)
          w.store_validity(validity, base);
      }
    }
    if (lane == 0)
      b.statuses[it] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
  }
}

// ---- gather_parquet_dictionary_strings ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gather_strings_kernel(GatherBatch b)
{
  const int lane = lane_id();
  for (uint64_t it = first_item(); it < b.items; it += item_stride()) {
    RowWalk w;
    w.load(b, it, lane);
    const cgptr dict = to_global(uniform_ptr(b.dict_ptrs[it]));
    const uint64_t dict_bytes = uniform((uint64_t)b.dict_bytes[it]);
    const HC_GLOBAL int32_t* const doff = (const HC_GLOBAL int32_t*)uniform_ptr(b.dict_offsets[it]);
    const uint64_t byte_capacity = uniform((uint64_t)b.byte_capacities[it]);
    const Shape s = shape_of(b.level_ptrs != nullptr, w.num_indices, w.rows, uniform((uint64_t)b.offset_capacities[it]), 1);
    bool ok = s.ok;
    uint64_t total = 0; // wave-uniform
    for (uint64_t base = 0; ok && base < w.rows; base += kStep) {
      ok = w.step(base);
      if (ok) {
        int32_t from = 0, to = 0;
        if (w.indexed) {
          from = doff[w.index];
          to = doff[(uint64_t)w.index + 1];
        }
        const bool refused = w.indexed && entry_refused(w.index, from, to, dict_bytes);
        const uint64_t sums = wave_scan_add_u64(refused ? 0 : (uint64_t)(uint32_t)(to - from));
        total += last_lane(sums);
        ok = wave_ballot(refused) == 0 && !total_refused(total, byte_capacity);
      }
    }
    ok = ok && w.counted();
    if (ok) {
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
        uint64_t source = 0; // where the row's bytes lie in the dictionary
        if (w.indexed) {
          const int32_t from = doff[w.index];
          length = (uint32_t)(doff[(uint64_t)w.index + 1] - from);
          source = entry_at(w.index, (uint64_t)from);
        }
        const uint32_t ends = wave_scan_add_u32(length); // the row's end among the step's bytes
        const uint32_t begins = ends - length;
        const uint32_t step_bytes = last_lane(ends);
        if (base + (uint64_t)lane < w.rows)
          out[base + (uint64_t)lane + 1] = (int32_t)(written + ends);
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
            bytes[(uint64_t)written + j] = dict[src + (j - begin)];
        }
        written += step_bytes;
        if (validity)
          w.store_validity(validity, base);
      }
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

template <class U, bool kOne>
hipError_t gather_as(const GatherBatch& b, hipStream_t stream)
{
  gather_kernel<U, kOne><<<walk_groups((const void*)gather_kernel<U, kOne>, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

} // namespace

hipError_t launch_index(const IndexBatch& b, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  index_kernel<<<walk_groups((const void*)index_kernel, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

hipError_t launch_gather(const GatherBatch& b, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  if (b.entry_bytes < 1 || b.entry_bytes > kMaxEntryBytes)
    return hipErrorInvalidValue;
  if (b.entry_bytes == 8)
    return gather_as<uint64_t, true>(b, stream);
  if (b.entry_bytes == 4)
    return gather_as<uint32_t, true>(b, stream);
  return b.entry_bytes % 4 == 0 ? gather_as<uint32_t, false>(b, stream) : gather_as<uint8_t, false>(b, stream);
}

hipError_t launch_gather_strings(const GatherBatch& b, hipStream_t stream)
{
  if (b.items == 0)
    return hipSuccess;
  gather_strings_kernel<<<walk_groups((const void*)gather_strings_kernel, b.items), kBlock, 0, stream>>>(b);
  return hipGetLastError();
}

} // namespace pqg
} // namespace hcamd
