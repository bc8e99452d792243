// zstd_kernels.hip -- batched Zstandard (RFC 8878) decoder for gfx950, one chunk per wavefront.
//
// Shape:
//   * kWavesPerBlock waves per workgroup, each with its own slice of LDS and its own literal buffer in the temp
//     space; the waves share nothing and never meet at a barrier.  Chunks are taken grid-stride.
//   * The decoder of a chunk is zstd_decode.hiph, shared with the kernels for frames that use dictionaries
//     (../zstd_dict/zstd_dict_kernels.hip) and instantiated here with DICT = false: a frame with a non-zero
//     Dictionary_ID is refused.
#include <hip/hip_runtime.h>

#include "zstd_decode.hiph"

namespace hcamd {
namespace {

__global__ __launch_bounds__(kWave* kWavesPerBlock) void zstd_decompress_kernel(
    const uint8_t* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes,
    const size_t* __restrict__ out_caps, const size_t batch, uint8_t* const* __restrict__ out_ptrs,
    size_t* __restrict__ actual_bytes, hipcompStatus_t* __restrict__ statuses, uint8_t* temp, const uint64_t lit_cap)
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
    uint64_t produced = 0;
    const bool ok = decode_chunk<true, false>(comp, comp_len, out, cap, lit, lit_cap, lds, lane, produced);
    if (lane == 0) {
      if (actual_bytes != nullptr)
        actual_bytes[chunk] = ok ? produced : 0;
      if (statuses != nullptr)
        statuses[chunk] = ok ? hipcompSuccess : hipcompErrorCannotDecompress;
    }
  }
}

// The size query.  Where every frame of the chunk declares its content size: their sum, the headers walked and
// nothing decoded.  Otherwise the decode without an output.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void zstd_sizes_kernel(
    const uint8_t* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes, const size_t batch,
    size_t* __restrict__ out_sizes)
{
  __shared__ WaveLds lds_all[kWavesPerBlock];
  const int lane = lane_id();
  const uint32_t wave = uniform((uint32_t)(threadIdx.x >> 6));
  WaveLds& lds = lds_all[wave];
  const size_t waves = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t chunk = (size_t)blockIdx.x * kWavesPerBlock + wave; chunk < batch; chunk += waves) {
    const uint8_t* comp_generic = uniform_ptr(comp_ptrs[chunk]);
    const uint64_t n = uniform((uint64_t)comp_bytes[chunk]);
    cgptr comp = to_global(comp_generic);
    uint64_t at = 0, total = 0;
    bool declared = true, good = true;
    while (at < n) {
      const FrameHeader fh = parse_frame_header(UBytes{comp + at}, n - at);
      if (fh.kind == kNoFrame) {
        good = false;
        break;
      }
      if (fh.kind == kSkippableFrame) {
        at += fh.skip_bytes;
        continue;
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
      good = decode_chunk<false, false>(comp_generic, n, nullptr, ~(uint64_t)0, nullptr, ~(uint64_t)0, lds, lane, produced);
      total = produced;
    }
    if (lane == 0)
      out_sizes[chunk] = good ? total : 0;
  }
}

unsigned grid_for(size_t batch)
{
  const uint64_t waves = waves_for(batch);
  return (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
}

} // namespace

void zstd_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps, size_t batch,
    size_t max_chunk_bytes_of_temp, void* temp, uint8_t* const* out_ptrs, size_t* actual_bytes, hipcompStatus_t* statuses,
    hipStream_t stream)
{
  zstd_decompress_kernel<<<dim3(grid_for(batch)), dim3(kWave * kWavesPerBlock), 0, stream>>>(
      comp_ptrs, comp_bytes, out_caps, batch, out_ptrs, actual_bytes, statuses, static_cast<uint8_t*>(temp),
      (uint64_t)max_chunk_bytes_of_temp);
}

void zstd_launch_get_sizes(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t* out_sizes, size_t batch, hipStream_t stream)
{
  zstd_sizes_kernel<<<dim3(grid_for(batch)), dim3(kWave * kWavesPerBlock), 0, stream>>>(comp_ptrs, comp_bytes, batch, out_sizes);
}

} // namespace hcamd
