// zstd_dict_compress_kernels.hip -- the Zstandard encoder kernels for frames that use dictionaries
// (include/hipcomp/zstd_dict_compress.h), for gfx950, one chunk or one dictionary per wavefront.
//
// Shape: the compress kernel is that of ../zstd_compress/zstd_compress_kernels.hip with one
// more argument, the chunks' prepared dictionaries; the chunk encoder is ../zstd_compress/zstd_encode.hiph,
// instantiated here with DICT = true.  It takes the same launch shape, the same LDS (EncLds) and the same temp
// space.  The prepare kernel digests a dictionary into its blob (zstd_dict_codes.hpp): the verdict, the match table
// primed with the tail by atomicMax in LDS, the dictionary's encoding tables built by the code the CPU driver
// runs, the tail.  A dictionary is read in [dict, dict + n) only and only its blob is written, with vector stores.
#include <hip/hip_runtime.h>

#include "zstd_encode.hiph"
#include "zstd_dict_compress_launch.hpp"

namespace hcamd {
namespace {

__global__ __launch_bounds__(kWave) void zstd_dict_compress_kernel(
    const uint8_t* const* __restrict__ in_ptrs, const size_t* __restrict__ in_bytes, const uint32_t max_chunk,
    const size_t batch, uint8_t* __restrict__ temp, const uint32_t records_per_wave, const uint32_t temp_per_wave,
    uint8_t* const* __restrict__ out_ptrs, size_t* __restrict__ out_bytes, const uint8_t* const* __restrict__ prepared,
    const uint32_t checksum)
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
    const uint8_t* blob = uniform_ptr(prepared[chunk]);
    // (a chunk above the limit the call was given: neither its records nor its frame would have room)
    const uint32_t c = size <= (size_t)max_chunk ? zstd_chunk<true>(src, (uint32_t)size, dst, rec_a, rec_b, lits, checksum != 0u, lds, lane, blob) : 0u;
    if (lane == 0)
      out_bytes[chunk] = c;
    lds_phase();
    global_phase();
  }
}

struct PrepareLds
{
  alignas(16) uint32_t table[kEncHashEntries]; // 32-bit for atomicMax; narrowed on the way out
  alignas(16) DictTables tables;
  DictScratch scratch;
  uint32_t logs[3];
  uint32_t verdict[16]; // DictLayout, word for word, from lane 0
};
static_assert(sizeof(DictTables) % 16 == 0, "the tables leave in 16-byte stores");

// bytes of global memory for the host's format logic on one lane
struct LaneBytes
{
  cgptr p;
  __device__ __forceinline__ uint8_t operator[](uint64_t i) const { return p[i]; }
  __device__ __forceinline__ LaneBytes operator+(uint64_t i) const { return LaneBytes{p + i}; }
};

__device__ __forceinline__ void store_16(gptr to, u32x4 v) { *reinterpret_cast<HC_GLOBAL u32x4*>(to) = v; }

// One wave per dictionary, grid-stride.
__global__ __launch_bounds__(kWave) void zstd_dict_compress_prepare_kernel(
    const uint8_t* const* __restrict__ dict_ptrs, const size_t* __restrict__ dict_bytes, const size_t count,
    uint8_t* const* __restrict__ prepared_ptrs, const size_t* __restrict__ prepared_caps, hipcompStatus_t* __restrict__ statuses)
{
  __shared__ PrepareLds lds;
  const int lane = (int)threadIdx.x;
  for (size_t i = blockIdx.x; i < count; i += gridDim.x) {
    cgptr src = to_global(uniform_ptr(dict_ptrs[i]));
    const uint64_t n64 = uniform((uint64_t)dict_bytes[i]);
    uint8_t* blob_generic = uniform_ptr(prepared_ptrs[i]);
    gptr blob = to_global(blob_generic);
    const uint64_t cap = uniform((uint64_t)prepared_caps[i]);
    EncBlobHeader h = invalid_blob_header();
    hipcompStatus_t status = hipcompSuccess;
    const bool aligned = (reinterpret_cast<uintptr_t>(blob_generic) & (kEncBlobAlign - 1u)) == 0;
    if (!aligned || (n64 <= kDictBytesMax && cap < enc_prepared_bytes(n64))) {
      status = hipcompErrorInvalidValue;
    } else if (n64 > kDictBytesMax) {
      status = hipcompErrorCannotDecompress;
    } else {
      const uint32_t n = (uint32_t)n64;
      const LaneBytes p{src};
      // ---- the verdict and the encoding tables: the host's code on lane 0
      for (uint32_t k = (uint32_t)lane; k < sizeof(DictTables) / 4u; k += kWave)
        reinterpret_cast<uint32_t*>(&lds.tables)[k] = 0u;
      for (uint32_t k = (uint32_t)lane; k < kEncHashEntries; k += kWave)
        lds.table[k] = 0u;
      lds_phase();
      if (lane == 0) {
        const DictLayout d = dict_verdict(p, n, lds.scratch);
        uint32_t logs[3] = {0, 0, 0};
        if (d.ok && d.formatted)
          build_dict_tables(p, n, d, lds.scratch, lds.tables, logs);
        lds.logs[0] = logs[0];
        lds.logs[1] = logs[1];
        lds.logs[2] = logs[2];
        lds.verdict[0] = d.ok;
        lds.verdict[1] = d.formatted;
        lds.verdict[2] = d.dict_id;
        lds.verdict[3] = d.content_at;
        lds.verdict[4] = d.content_size;
        lds.verdict[5] = d.rep[0];
        lds.verdict[6] = d.rep[1];
        lds.verdict[7] = d.rep[2];
      }
      lds_phase();
      if (uniform(lds.verdict[0]) == 0u) {
        status = hipcompErrorCannotDecompress;
      } else {
        const uint32_t content_at = uniform(lds.verdict[3]), content_size = uniform(lds.verdict[4]);
        const uint32_t t = tail_of(content_size);
        cgptr tail = src + content_at + (content_size - t);
        // ---- the primed table: the greatest position of every slot
        for (uint32_t v = (uint32_t)lane; v + 4u <= t; v += kWave)
          atomicMax(&lds.table[hash_of(load_u32_any(tail + v))], v);
        lds_phase();
        for (uint32_t k = (uint32_t)lane; k < kEncHashEntries / 8u; k += kWave) {
          const uint32_t* e = &lds.table[8u * k];
          const u32x4 v = {e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
          store_16(blob + kEncBlobTable + 16u * k, v);
        }
        for (uint32_t k = (uint32_t)lane; k < sizeof(DictTables) / 16u; k += kWave)
          store_16(blob + kEncBlobTables + 16u * k, reinterpret_cast<const u32x4*>(&lds.tables)[k]);
        // ---- the tail, zeros to the blob's end
        const uint32_t units = ((uint32_t)enc_prepared_bytes(n64) - kEncBlobTail) / 16u;
        for (uint32_t u = (uint32_t)lane; u < units; u += kWave) {
          const uint32_t base = 16u * u;
          u32x4 v = {0, 0, 0, 0};
          if (base + 16u <= t) {
            v.x = load_u32_any(tail + base);
            v.y = load_u32_any(tail + base + 4u);
            v.z = load_u32_any(tail + base + 8u);
            v.w = load_u32_any(tail + base + 12u);
          } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 16u; ++b)
              if (base + b < t)
                w[b >> 2] |= (uint32_t)tail[base + b] << (8u * (b & 3u));
            v.x = w[0];
            v.y = w[1];
            v.z = w[2];
            v.w = w[3];
          }
          store_16(blob + kEncBlobTail + base, v);
        }
        h.valid = 1;
        h.dict_id = uniform(lds.verdict[2]);
        h.has_entropy = uniform(lds.verdict[1]);
        h.rep[0] = uniform(lds.verdict[5]);
        h.rep[1] = uniform(lds.verdict[6]);
        h.rep[2] = uniform(lds.verdict[7]);
        h.content_size = content_size;
        h.tail = t;
        h.ll_log = uniform(lds.logs[0]);
        h.of_log = uniform(lds.logs[1]);
        h.ml_log = uniform(lds.logs[2]);
      }
    }
    // ---- the header last, from lane 0
    if (aligned && cap >= sizeof(EncBlobHeader) && lane == 0) {
      const uint32_t words[16] = {h.magic,  h.version,      h.valid, h.dict_id, h.has_entropy, h.rep[0], h.rep[1], h.rep[2],
                                  h.content_size, h.tail, h.ll_log, h.of_log,  h.ml_log,      0u,       0u,       0u};
      static_assert(sizeof words == sizeof(EncBlobHeader), "the header word for word");
      HC_GLOBAL uint32_t* to = reinterpret_cast<HC_GLOBAL uint32_t*>(blob);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        to[k] = words[k];
    }
    if (lane == 0)
      statuses[i] = status;
    lds_phase();
  }
}

} // namespace

void zstd_dict_compress_launch_prepare(
    const uint8_t* const* dict_ptrs, const size_t* dict_bytes, size_t count, uint8_t* const* prepared_ptrs,
    const size_t* prepared_caps, hipcompStatus_t* statuses, hipStream_t stream)
{
  zstd_dict_compress_prepare_kernel<<<dim3((unsigned)zstd::enc_waves_for(count)), dim3(kWave), 0, stream>>>(
      dict_ptrs, dict_bytes, count, prepared_ptrs, prepared_caps, statuses);
}

void zstd_dict_compress_launch(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t max_chunk_bytes, size_t batch, void* temp,
    uint8_t* const* out_ptrs, size_t* out_bytes, const uint8_t* const* prepared, bool checksum, hipStream_t stream)
{
  zstd_dict_compress_kernel<<<dim3((unsigned)zstd::enc_waves_for(batch)), dim3(kWave), 0, stream>>>(
      in_ptrs, in_bytes, (uint32_t)max_chunk_bytes, batch, reinterpret_cast<uint8_t*>(temp),
      (uint32_t)zstd::enc_records_per_wave(max_chunk_bytes), (uint32_t)zstd::enc_temp_bytes_per_wave(max_chunk_bytes), out_ptrs,
      out_bytes, prepared, checksum ? 1u : 0u);
}

} // namespace hcamd
