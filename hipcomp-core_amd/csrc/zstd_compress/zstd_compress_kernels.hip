// zstd_compress_kernels.hip -- batched Zstandard (RFC 8878) encoder for gfx950, one chunk per wavefront.
//
// Shape:
//   * One wave per workgroup with its own LDS; chunks are taken grid-stride, so the grid -- and with it the temp
//     space, one set of buffers per wave -- is bounded whatever the batch.  Waves share nothing and never wait for
//     one another.
//   * Parse: the Deflate encoder's greedy LZ77, 64 positions per trip: every lane hashes the 4 bytes at its position,
//     looks its slot of a 4096-entry table of 16-bit positions up, validates the candidate by comparing the 4
//     bytes, a ballot picks the first hit; the match is extended 64 bytes per step to the chunk's end.  Sequences
//     leave as two 32-bit records (literal run | offset << 16; match length) to the wave's buffers in temp space,
//     the literal bytes are gathered behind one another in the wave's literal buffer, the literal histogram is
//     counted in LDS as the parse goes.
//   * Codes: zstd_codes.hpp.  The sort of the literal histogram runs over the lanes (rank_of), the code lengths,
//     the tree's description, the three tables' modes and their encoding tables on one lane.
//   * Sizes before bytes: the literals section's size is exact before it is written (the streams' bits are summed
//     first); the sequences' bitstream is written behind it with a limit that keeps the block below the chunk's
//     size, and where it would pass it the frame is written again as a Raw_Block.
//   * Literals: per trip 64 symbols from the stream's end down; a prefix sum of the code lengths places every
//     lane's code with ds_or_b32 into a zeroed LDS stage, whole dwords of which leave with one store per lane.
//   * Sequences: lanes 0, 1, 2 walk the three FSE state chains, last sequence first, one table each; every step's
//     (bits, count) goes to the lane that owns the sequence, which adds its extra bits, and a prefix sum places 64
//     sequences per trip in the stage.
//   * Bounds: a chunk reads [src, src + len) and its own buffers, and writes at most len + 14 bytes.
//
// The chunk encoder itself is zstd_encode.hiph, shared with ../zstd_dict_compress and instantiated here with
// DICT = false.
#include <hip/hip_runtime.h>

#include "zstd_encode.hiph"

namespace hcamd {
namespace {

__global__ __launch_bounds__(kWave) void zstd_compress_kernel(
    const uint8_t* const* __restrict__ in_ptrs, const size_t* __restrict__ in_bytes, const uint32_t max_chunk,
    const size_t batch, uint8_t* __restrict__ temp, const uint32_t records_per_wave, const uint32_t temp_per_wave,
    uint8_t* const* __restrict__ out_ptrs, size_t* __restrict__ out_bytes, const uint32_t checksum)
{
  __shared__ EncLds lds;
  const int lane = (int)threadIdx.x;
  uint8_t* mine = temp + (size_t)blockIdx.x * temp_per_wave;
  uint32_t* rec_a = reinterpret_cast<uint32_t*>(mine);
  uint32_t* rec_b = rec_a + records_per_wave;
  uint8_t* lits = reinterpret_cast<uint8_t*>(rec_b + records_per_wave);
  for (size_t chunk = blockIdx.x; chunk < batch; chunk += gridDim.x) {
    cgptr src = to_global(uniform_ptr(in_ptrs[chunk]));
    const size_t size = (size_t)uniform((uint64_t)in_bytes[chunk]);
    gptr dst = to_global(uniform_ptr(out_ptrs[chunk]));
    // (a chunk above the limit the call was given: neither its records nor its frame would have room)
    const uint32_t c = size <= (size_t)max_chunk ? zstd_chunk<false>(src, (uint32_t)size, dst, rec_a, rec_b, lits, checksum != 0u, lds, lane) : 0u;
    if (lane == 0)
      out_bytes[chunk] = c;
    lds_phase();
    global_phase();
  }
}

} // namespace

void zstd_launch_compress(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t max_chunk_bytes, size_t batch, void* temp,
    uint8_t* const* out_ptrs, size_t* out_bytes, bool checksum, hipStream_t stream)
{
  zstd_compress_kernel<<<dim3((unsigned)zstd::enc_waves_for(batch)), dim3(kWave), 0, stream>>>(
      in_ptrs, in_bytes, (uint32_t)max_chunk_bytes, batch, reinterpret_cast<uint8_t*>(temp),
      (uint32_t)zstd::enc_records_per_wave(max_chunk_bytes), (uint32_t)zstd::enc_temp_bytes_per_wave(max_chunk_bytes), out_ptrs,
      out_bytes, checksum ? 1u : 0u);
}

} // namespace hcamd
