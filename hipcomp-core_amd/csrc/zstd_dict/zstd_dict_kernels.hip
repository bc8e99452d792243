// zstd_dict_kernels.hip -- the Zstandard kernels for frames that use dictionaries (include/hipcomp/zstd_dict.h),
// for gfx950, one chunk or one dictionary per wavefront.
//
// Shape: the decode and size kernels are those of ../zstd/zstd_kernels.hip with one more
// argument, the chunks' prepared dictionaries; the decoder itself is ../zstd/zstd_decode.hiph, instantiated here
// with DICT = true.  They take the same LDS (WaveLds) and the same temp space.  The prepare kernel digests a
// dictionary into its blob (zstd_dict.hpp): it builds the four tables in LDS exactly as a block does and stores
// them with the content.  Every path checks its bounds first; chunk i reads only its input and its blob, a
// dictionary is read in [dict, dict + n) only and only its blob is written.
#include <hip/hip_runtime.h>

#include "zstd/zstd_decode.hiph"
#include "zstd_dict_launch.hpp"

namespace hcamd {
namespace {

__global__ __launch_bounds__(kWave* kWavesPerBlock) void zstd_dict_decompress_kernel(
    const uint8_t* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes,
    const size_t* __restrict__ out_caps, const size_t batch, uint8_t* const* __restrict__ out_ptrs,
    size_t* __restrict__ actual_bytes, hipcompStatus_t* __restrict__ statuses, uint8_t* temp, const uint64_t lit_cap,
    const uint8_t* const* __restrict__ prepared)
{
  __shared__ WaveLds lds_all[kWavesPerBlock];
  const int lane = lane_id();
  const uint32_t wave = uniform((uint32_t)(threadIdx.x >> 6));
  WaveLds& lds = lds_all[wave];
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  const size_t me = (size_t)blockIdx.x * kWavesPerBlock + wave;
  uint8_t* lit = temp + me * lit_cap;
  for (size_t chunk = me; chunk < batch; chunk += waves) {
    const uint8_t* comp = uniform_ptr(comp_ptrs[chunk]);
    const uint64_t comp_len = uniform((uint64_t)comp_bytes[chunk]);
    uint8_t* out = uniform_ptr(out_ptrs[chunk]);
    const uint64_t cap = uniform((uint64_t)out_caps[chunk]);
    const uint8_t* blob = uniform_ptr(prepared[chunk]);
    uint64_t produced = 0;
    const bool ok = decode_chunk<true, true>(comp, comp_len, out, cap, lit, lit_cap, lds, lane, produced, blob);
    if (lane == 0) {
      if (actual_bytes != nullptr)
        actual_bytes[chunk] = ok ? produced : 0;
      if (statuses != nullptr)
        statuses[chunk] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
    }
  }
}

// The size query.  Where every frame of the chunk declares its content size: their sum, the headers walked with
// the Dictionary_ID rule and nothing decoded.  Otherwise the decode without an output, with the dictionary.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void zstd_dict_sizes_kernel(
    const uint8_t* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes, const size_t batch,
    size_t* __restrict__ out_sizes, const uint8_t* const* __restrict__ prepared)
{
  __shared__ WaveLds lds_all[kWavesPerBlock];
  const int lane = lane_id();
  const uint32_t wave = uniform((uint32_t)(threadIdx.x >> 6));
  WaveLds& lds = lds_all[wave];
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t chunk = (size_t)blockIdx.x * kWavesPerBlock + wave; chunk < batch; chunk += waves) {
    const uint8_t* comp_generic = uniform_ptr(comp_ptrs[chunk]);
    const uint64_t n = uniform((uint64_t)comp_bytes[chunk]);
    const uint8_t* blob = uniform_ptr(prepared[chunk]);
    cgptr comp = to_global(comp_generic);
    uint64_t at = 0, total = 0;
    bool declared = true;
    DictRef dict;
    bool good = dict_open(blob, dict);
    while (good && at < n) {
      const FrameHeader fh = parse_frame_header(UBytes{comp + at}, n - at, true);
      if (fh.kind == kNoFrame) {
        good = false;
        break;
      }
      if (fh.kind == kSkippableFrame) {
        at += fh.skip_bytes;
        continue;
      }
      if (!dict_id_accepted(fh.dict_id, dict.dict_id)) {
        good = false;
        break;
      }
      if (!fh.has_size) {
        declared = false;
        break;
      }
      at += fh.header_bytes;
      total += fh.content_size;
      for (;;) {
        const BlockHeader bh = parse_block_header(UBytes{comp + at}, n - at);
        if (!bh.ok) {
          good = false;
          break;
        }
        at += 3u + bh.comp_bytes;
        if (bh.last)
          break;
      }
      if (!good)
        break;
      if (fh.checksum) {
        if (n - at < 4) {
          good = false;
          break;
        }
        at += 4;
      }
    }
    if (good && !declared) {
      uint64_t produced = 0;
      good = decode_chunk<false, true>(comp_generic, n, nullptr, ~(uint64_t)0, nullptr, ~(uint64_t)0, lds, lane, produced, blob);
      total = produced;
    }
    if (lane == 0)
      out_sizes[chunk] = good ? total : 0;
  }
}

// lanes store table[0, count) of T to the blob, zeros behind `live` entries (what LDS holds there is not the table's)
template <class T>
__device__ __forceinline__ void store_table(gptr blob, uint32_t at, const T* table, uint32_t count, uint32_t live, int lane)
{
  HC_GLOBAL T* to = reinterpret_cast<HC_GLOBAL T*>(blob + at);
  for (uint32_t i = (uint32_t)lane; i < count; i += kWave)
    to[i] = i < live ? table[i] : T{};
}

__device__ __forceinline__ void store_header(gptr blob, const PreparedHeader& h, int lane)
{
  const uint32_t words[16] = {h.magic,  h.version, h.valid,  h.dict_id, h.has_entropy,    h.ll_log,       h.ml_log,     h.of_log,
                              h.huf_log, h.rep[0], h.rep[1], h.rep[2],  h.content_offset, h.content_size, h.total_size, h.reserved};
  static_assert(sizeof words == sizeof(PreparedHeader), "the header word for word");
  HC_GLOBAL uint32_t* to = reinterpret_cast<HC_GLOBAL uint32_t*>(blob);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      to[k] = words[k];
  }
}

// One wave per dictionary: the verdict (parse_dictionary), the four tables built in LDS as a block builds them
// (huf_sort / huf_entry, fse_build), stored to the blob with the content.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void zstd_dict_prepare_kernel(
    const uint8_t* const* __restrict__ dict_ptrs, const size_t* __restrict__ dict_bytes, const size_t count,
    uint8_t* const* __restrict__ prepared_ptrs, const size_t* __restrict__ prepared_caps, hipcompStatus_t* __restrict__ statuses)
{
  __shared__ WaveLds lds_all[kWavesPerBlock];
  const int lane = lane_id();
  const uint32_t wave = uniform((uint32_t)(threadIdx.x >> 6));
  WaveLds& lds = lds_all[wave];
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t i = (size_t)blockIdx.x * kWavesPerBlock + wave; i < count; i += waves) {
    cgptr src = to_global(uniform_ptr(dict_ptrs[i]));
    const uint64_t n64 = uniform((uint64_t)dict_bytes[i]);
    uint8_t* blob_generic = uniform_ptr(prepared_ptrs[i]);
    gptr blob = to_global(blob_generic);
    const uint64_t cap = uniform((uint64_t)prepared_caps[i]);
    PreparedHeader h{kPreparedMagic, kPreparedVersion, 0, 0, 0, 0, 0, 0, 0, {1, 4, 8}, kPreparedContent, 0, (uint32_t)sizeof(PreparedHeader), 0};
    hipcompStatus_t status = hipcompSuccess;
    const bool aligned = (reinterpret_cast<uintptr_t>(blob_generic) & (kPreparedAlign - 1u)) == 0;
    if (!aligned || (n64 <= kDictBytesMax && cap < prepared_bytes(n64))) {
      status = hipcompErrorInvalidValue;
    } else if (n64 > kDictBytesMax) {
      status = hipcompErrorCannotDecompress;
    } else {
      const uint32_t n = (uint32_t)n64;
      const UBytes p{src};
      const DictLayout d = parse_dictionary(p, n, lds.weights, lds.norm, lds.wt, lds.next);
      if (!d.ok) {
        status = hipcompErrorCannotDecompress;
      } else {
        if (d.formatted) {
          // (the descriptions passed parse_dictionary: they are read again, this time for their tables)
          const HufDesc hd = read_huf_weights(p + d.huf_at, n - d.huf_at, lds.weights, lds.norm, lds.wt, lds.next);
          huf_sort(lds.weights, hd.nsym, lds.hcount, lds.sorted);
          lds_phase();
          for (uint32_t e = (uint32_t)lane; e < (1u << hd.log); e += kWave)
            lds.huf[e] = (uint16_t)huf_entry(e, lds.hcount, lds.sorted, hd.log);
          const NCount of = read_ncount(p + d.of_at, n - d.of_at, lds.norm, kOFSymMax, kOFLogMax);
          fse_build(lds.norm, of.nsym, of.log, lds.of, lds.next);
          const NCount ml = read_ncount(p + d.ml_at, n - d.ml_at, lds.norm, kMLSymMax, kMLLogMax);
          fse_build(lds.norm, ml.nsym, ml.log, lds.ml, lds.next);
          const NCount ll = read_ncount(p + d.ll_at, n - d.ll_at, lds.norm, kLLSymMax, kLLLogMax);
          fse_build(lds.norm, ll.nsym, ll.log, lds.ll, lds.next);
          lds_phase();
          store_table(blob, kPreparedLL, reinterpret_cast<const uint32_t*>(lds.ll), 1u << kLLLogMax, 1u << ll.log, lane);
          store_table(blob, kPreparedML, reinterpret_cast<const uint32_t*>(lds.ml), 1u << kMLLogMax, 1u << ml.log, lane);
          store_table(blob, kPreparedOF, reinterpret_cast<const uint32_t*>(lds.of), 1u << kOFLogMax, 1u << of.log, lane);
          store_table(blob, kPreparedHuf, lds.huf, 1u << kHufLogMax, 1u << hd.log, lane);
          lds_phase();
          h.has_entropy = 1;
          h.ll_log = ll.log;
          h.ml_log = ml.log;
          h.of_log = of.log;
          h.huf_log = hd.log;
        }
        wave_copy(blob + kPreparedContent, src + d.content_at, d.content_size, lane);
        h.valid = 1;
        h.dict_id = d.dict_id;
        h.rep[0] = d.rep[0];
        h.rep[1] = d.rep[1];
        h.rep[2] = d.rep[2];
        h.content_size = d.content_size;
        h.total_size = (uint32_t)prepared_bytes(n64);
      }
    }
    if (aligned && cap >= sizeof(PreparedHeader))
      store_header(blob, h, lane);
    if (lane == 0)
      statuses[i] = status;
  }
}

unsigned grid_for(size_t batch)
{
  const uint64_t waves = waves_for(batch);
  return (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
}

} // namespace

void zstd_dict_launch_prepare(
    const uint8_t* const* dict_ptrs, const size_t* dict_bytes, size_t count, uint8_t* const* prepared_ptrs,
    const size_t* prepared_caps, hipcompStatus_t* statuses, hipStream_t stream)
{
  zstd_dict_prepare_kernel<<<dim3(grid_for(count)), dim3(kWave * kWavesPerBlock), 0, stream>>>(
      dict_ptrs, dict_bytes, count, prepared_ptrs, prepared_caps, statuses);
}

void zstd_dict_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps, size_t batch,
    size_t max_chunk_bytes_of_temp, void* temp, uint8_t* const* out_ptrs, size_t* actual_bytes, hipcompStatus_t* statuses,
    const uint8_t* const* prepared, hipStream_t stream)
{
  zstd_dict_decompress_kernel<<<dim3(grid_for(batch)), dim3(kWave * kWavesPerBlock), 0, stream>>>(
      comp_ptrs, comp_bytes, out_caps, batch, out_ptrs, actual_bytes, statuses, static_cast<uint8_t*>(temp),
      (uint64_t)max_chunk_bytes_of_temp, prepared);
}

void zstd_dict_launch_get_sizes(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const uint8_t* const* prepared, size_t* out_sizes, size_t batch,
    hipStream_t stream)
{
  zstd_dict_sizes_kernel<<<dim3(grid_for(batch)), dim3(kWave * kWavesPerBlock), 0, stream>>>(
      comp_ptrs, comp_bytes, batch, out_sizes, prepared);
}

} // namespace hcamd
