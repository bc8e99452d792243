// hlif.hip -- the high-level interface (include/hipcomp/hipcompManager.hpp, lz4.hpp, snappy.hpp,
// cascaded.hpp, hipcompManagerFactory.hpp, hlif.h): one container per buffer, written and read
// on the device over the batched kernels of the three codecs.
//
// Reference: src/highlevel/{ManagerBase,BatchManager,LZ4Manager,SnappyManager,CascadedManager}.hpp,
// hipcompManagerFactory.cpp, the persistent-CTA
// loop of src/hipcomp_common_deps/hlif_shared.hiph:165-232 (each CTA compresses a chunk into
// its scratch slot, claims room in the container with an atomic on comp_data_size and copies
// the chunk there: chunk data in completion order) and :293-345.
// Here: the same scheme inside the batched encoders of all three codecs -- a wave compresses into a slot of its
// own (one per RESIDENT wave, not per chunk), takes the chunk's room in the container with an atomic add on
// comp_data_size when the size is known, and copies it there (placement.hpp); an LZ4 chunk that ends in one
// long literal run (data that does not compress) takes its room before that run is written and writes it in
// place, once (lz4_common.hiph: reserve_place).  Chunk data in completion order, as in the reference.  No
// stream, event or thread of the manager's own: everything runs on the caller's stream.  The scratch space is a
// constant of the manager, as in the reference.
#include "cascaded_launch.hpp"
#include "checksum_launch.hpp"
#include "gather_launch.hpp"
#include "hlif_container.hpp"
#include "host_common.hpp"
#include "lz4_frame_index_launch.hpp"
#include "lz4_frame_launch.hpp"
#include "lz4_frames_launch.hpp"
#include "lz4_launch.hpp"
#include "parquet_delta_launch.hpp"
#include "parquet_dict_launch.hpp"
#include "parquet_plain_launch.hpp"
#include "parquet_hybrid_launch.hpp"
#include "parquet_pages_launch.hpp"
#include "range_launch.hpp"
#include "snappy_frame_index_launch.hpp"
#include "snappy_frame_launch.hpp"
#include "snappy_launch.hpp"
#include "wave_utils.hpp"

#include "hipcomp/cascaded.h"
#include "hipcomp/cascaded.hpp"
#include "hipcomp/hipcompManagerFactory.hpp"
#include "hipcomp/hlif.h"
#include "hipcomp/lz4.h"
#include "hipcomp/lz4.hpp"
#include "hipcomp/snappy.h"
#include "hipcomp/snappy.hpp"

#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

namespace hcamd {
namespace hlif {

// format headers behind the common one (reference include/hipcomp/{lz4,snappy,cascaded}.hpp):
// LZ4 {hipcompType_t} 4 bytes, Snappy {} 1 byte (an empty struct), Cascaded {options} 24 bytes
constexpr size_t kMaxFormatHeaderBytes = 24;
struct FormatHeader
{
  uint8_t bytes[kMaxFormatHeaderBytes];
};

// where the arrays and the chunk data of a container of n chunks start (bytes from its start;
// the reference aligns the ADDRESS behind the two headers to 8 -- containers are at least
// 8-byte aligned, so that is an offset)
struct Layout
{
  size_t offsets, sizes, comp_checksums, decomp_checksums, data;
};
inline Layout layout_of(size_t n, size_t format_header_bytes)
{
  Layout l;
  l.offsets = (sizeof(CommonHeader) + format_header_bytes + 7) & ~size_t(7);
  l.sizes = l.offsets + 8 * n;
  l.comp_checksums = l.sizes + 8 * n;
  l.decomp_checksums = l.comp_checksums + 4 * n;
  l.data = l.decomp_checksums + 4 * n;
  return l;
}

constexpr int kBlock = 256;

// ---- compression ------------------------------------------------------------------------
__global__ void header_kernel(
    uint8_t* container, uint64_t decomp_bytes, uint64_t num_chunks, uint64_t chunk_bytes, uint32_t data_offset,
    uint8_t format, FormatHeader format_header, uint32_t format_header_bytes, hipcompStatus_t* status)
{
  CommonHeader* h = reinterpret_cast<CommonHeader*>(container);
  h->magic_number = 0; // reference fill_common_header, hlif_shared.hiph:113-131
  h->major_version = 2;
  h->minor_version = 2;
  h->format = format;
  h->comp_data_size = 0;
  h->decomp_data_size = decomp_bytes;
  h->num_chunks = num_chunks;
  h->include_chunk_starts = true;
  h->full_comp_buffer_checksum = 0;
  h->decomp_buffer_checksum = 0;
  h->include_per_chunk_comp_buffer_checksums = false;
  h->include_per_chunk_decomp_buffer_checksums = false;
  h->uncomp_chunk_size = chunk_bytes;
  h->comp_data_offset = data_offset;
  for (uint32_t i = 0; i < format_header_bytes; ++i)
    container[sizeof(CommonHeader) + i] = format_header.bytes[i];
  if (status)
    *status = hipcompSuccess;
}

// chunk list of one pass: inputs are slices of the buffer; the pass's chunk ticket counter = 0 (the Snappy /
// Cascaded kernels draw their chunks from it; zeroed here, by a kernel on the stream, not by hipMemsetAsync:
// lz4_kernels.hip, lz4_launch_decompress, says what was seen with a memset node in a captured graph)
__global__ void slab_inputs_kernel(
    const uint8_t* decomp, uint64_t decomp_bytes, uint64_t chunk_bytes, uint64_t first, uint32_t count,
    const uint8_t** in_ptrs, size_t* in_bytes, uint32_t* ticket)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0)
    *ticket = 0;
  if (i >= count)
    return;
  const uint64_t at = (first + i) * chunk_bytes;
  in_ptrs[i] = decomp + at;
  in_bytes[i] = (size_t)(decomp_bytes - at < chunk_bytes ? decomp_bytes - at : chunk_bytes);
}

// ---- decompression ------------------------------------------------------------------------
// The header is the container's own word about itself and may be corrupt or hostile: the
// chunk list of a slab is made only if it agrees with what the manager and the caller's
// configuration say (format, chunk size, chunk count, size of the output, where the data
// starts) -- otherwise every chunk of the slab gets an empty output slice and a one-byte
// stream, fails, and the verdict kernel reports hipcompErrorCannotDecompress.  Either way no
// output slice reaches past decomp_bytes.
__global__ void slab_streams_kernel(
    const uint8_t* container, uint64_t offsets_at, uint8_t* decomp, uint64_t decomp_bytes,
    uint64_t chunk_bytes, uint64_t first, uint32_t count, uint64_t num_chunks, uint32_t format, uint64_t data_at,
    const uint8_t** comp_ptrs, uint8_t** out_ptrs, size_t* caps, hipcompStatus_t* status)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count)
    return;
  const CommonHeader* h = reinterpret_cast<const CommonHeader*>(container);
  const bool header_ok = h->format == format && h->uncomp_chunk_size == chunk_bytes
                         && h->num_chunks == num_chunks && h->decomp_data_size == decomp_bytes
                         && h->comp_data_offset == data_at
                         && num_chunks == (decomp_bytes + chunk_bytes - 1) / chunk_bytes;
  const uint64_t off = reinterpret_cast<const uint64_t*>(container + offsets_at)[first + i];
  const uint64_t at = (first + i) * chunk_bytes;
  if (!header_ok) {
    comp_ptrs[i] = container;
    out_ptrs[i] = decomp;
    caps[i] = 0;
    *status = hipcompErrorCannotDecompress;
    return;
  }
  comp_ptrs[i] = container + data_at + off;
  out_ptrs[i] = decomp + at;
  caps[i] = at >= decomp_bytes ? 0 : (size_t)(decomp_bytes - at < chunk_bytes ? decomp_bytes - at : chunk_bytes);
}

// a chunk that failed, or did not fill its slice, fails the whole buffer
__global__ void slab_verdict_kernel(
    const hipcompStatus_t* statuses, const size_t* actual, const size_t* caps, uint32_t count, hipcompStatus_t* status)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < count && (statuses[i] != hipcompSuccess || actual[i] != caps[i]))
    *status = hipcompErrorCannotDecompress;
}

__global__ void set_status_kernel(hipcompStatus_t* status, hipcompStatus_t value) { *status = value; }

inline void check(hipError_t e, const char* what)
{
  if (e != hipSuccess)
    throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// The status word of a configuration (pinned host memory: kernels write it, the host reads it).  A
// configuration is made per call in the reference's API; hipHostMalloc + hipHostFree per call were a fifth of a
// 3 ms compress.  Words come from pages of 64 that are handed out again and never given back (a process that
// configures holds a few hundred bytes of pinned memory until it ends; the list is leaked on purpose: a
// configuration in a static of the caller's may outlive this library's own statics).
struct StatusPool
{
  std::mutex lock;
  std::vector<hipcompStatus_t*> spare;
  hipcompStatus_t* take()
  {
    std::lock_guard<std::mutex> g(lock);
    if (spare.empty()) {
      hipcompStatus_t* page = nullptr;
      check(hipHostMalloc((void**)&page, 64 * sizeof(hipcompStatus_t), hipHostMallocDefault), "hipHostMalloc(status)");
      for (int i = 0; i < 64; ++i)
        spare.push_back(page + i);
    }
    hipcompStatus_t* p = spare.back();
    spare.pop_back();
    return p;
  }
  void give(hipcompStatus_t* p)
  {
    std::lock_guard<std::mutex> g(lock);
    spare.push_back(p);
  }
};
inline StatusPool& status_pool()
{
  static StatusPool* pool = new StatusPool;
  return *pool;
}
inline std::shared_ptr<hipcompStatus_t> new_status()
{
  hipcompStatus_t* p = status_pool().take();
  *p = hipcompSuccess;
  return std::shared_ptr<hipcompStatus_t>(p, [](hipcompStatus_t* q) { status_pool().give(q); });
}

// What the three managers share: the container, the slabs, the scratch space.  The codec is
// a small set of hooks.
struct Core
{
  enum Codec { LZ4, Snappy, Cascaded } codec;
  size_t chunk_bytes = 0;
  hipStream_t stream = nullptr;
  size_t slot_bytes = 0;   // hipcompBatched*CompressGetMaxOutputChunkSize(chunk_bytes), 16-byte multiple
  uint32_t slab = 0;       // chunks per pass of decompress
  uint8_t format = kLZ4;
  FormatHeader format_header = {};
  uint32_t format_header_bytes = 0;
  uint32_t place_align = 1; // chunk starts in the container
  // LZ4
  hipcompType_t lz4_type = HIPCOMP_TYPE_CHAR;
  int lz4_elem = 1;
  uint32_t ht_size = 0;
  // Cascaded
  hipcompBatchedCascadedOpts_t cascaded_opts = {};
  int cascaded_elem = 4;

  // CRC-32 checksums (checksum_launch.hpp): what compress writes and decompress checks
  hipcomp::ChecksumPolicy policy = hipcomp::NoComputeNoVerify;
  bool computes() const
  {
    return policy == hipcomp::ComputeAndNoVerify || policy == hipcomp::ComputeAndVerifyIfPresent
           || policy == hipcomp::ComputeAndVerify;
  }
  bool verifies() const
  {
    return policy == hipcomp::NoComputeAndVerifyIfPresent || policy == hipcomp::ComputeAndVerifyIfPresent
           || policy == hipcomp::ComputeAndVerify;
  }
  void set_policy(hipcomp::ChecksumPolicy p)
  {
    if (p < hipcomp::NoComputeNoVerify || p > hipcomp::ComputeAndVerify)
      throw std::runtime_error("unknown ChecksumPolicy " + std::to_string((int)p));
    policy = p;
  }

  uint8_t* scratch = nullptr;
  bool own_scratch = false;
  CommonHeader* header_host = nullptr; // pinned
  Core(Codec c, size_t chunk, hipStream_t st, int device_id, const char* who) : codec(c), chunk_bytes(chunk), stream(st)
  {
    int dev = -1;
    check(hipGetDevice(&dev), "hipGetDevice");
    if (dev != device_id)
      throw std::runtime_error(std::string(who) + ": device_id " + std::to_string(device_id) + " is not the current device");
    check(hipHostMalloc((void**)&header_host, sizeof(CommonHeader), hipHostMallocDefault), "hipHostMalloc(header)");
  }
  ~Core()
  {
    if (own_scratch)
      (void)hipFree(scratch);
    (void)hipHostFree(header_host);
    if (ranges_head_host)
      (void)hipHostFree(ranges_head_host);
  }
  Core(const Core&) = delete;
  Core& operator=(const Core&) = delete;

  void finish_init(size_t max_compressed_chunk)
  {
    slot_bytes = (max_compressed_chunk + 15) & ~size_t(15);
    slab = (uint32_t)kPlacedSlab;
  }

  Layout layout(size_t n) const { return layout_of(n, format_header_bytes); }

  // decompress: the chunk lists of a pass (and 64 spare bytes: the LZ4 decoder's ticket counter)
  size_t lists_bytes() const { return (size_t)slab * (8 + 8 + 8 + 8 + 8 + 4) + 64; }
  // compress: the encoders place the chunks themselves (placement.hpp) -- a slot per resident wave, no scan, no
  // gather, no second stream; a pass takes up to kPlacedSlab chunks (what bounds it is the chunk lists and the
  // LZ4 launcher's routing lists, 40 bytes per chunk).  Scratch: the pass's input list, 64 spare bytes (the
  // Snappy / Cascaded kernels' ticket counter), the slots, and the LZ4 launcher's own temp space (its header,
  // routing lists and hash tables: lz4_launch.hpp).
  static constexpr size_t kPlacedSlab = 262144;
  size_t lz4_temp_bytes(size_t chunks) const { return codec == LZ4 ? lz4_compress_temp_bytes_used(ht_size, chunks) : 0; }
  size_t placement_slots() const
  {
    const size_t n = codec == LZ4      ? lz4_placement_slots()
                     : codec == Snappy ? snappy_placement_slots()
                                       : cascaded_placement_slots(cascaded_elem);
    if (n == 0)
      throw std::runtime_error("compress: cannot find out how many workgroups the device holds");
    return n;
  }
  size_t placed_scratch_bytes(size_t chunks) const
  {
    return 16 * chunks + 64 + placement_slots() * slot_bytes + 16 + lz4_temp_bytes(chunks);
  }
  // the checksums of a pass (behind what the pass needs without them, 16-byte aligned): the CrcState, the scan
  size_t checksum_bytes(size_t chunks) const
  {
    return policy == hipcomp::NoComputeNoVerify ? 0 : 16 + 64 + crc_pass_bytes(chunks);
  }
  static uint8_t* checksum_area(uint8_t* behind)
  {
    return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(behind) + 15) & ~uintptr_t(15));
  }
  // bytes of the uncompressed buffer that chunks [first, first + count) cover
  uint64_t slice_bytes(uint64_t total, size_t first, size_t count) const
  {
    const uint64_t end = (uint64_t)(first + count) * chunk_bytes;
    return (end < total ? end : total) - (uint64_t)first * chunk_bytes;
  }
  // what a caller's own scratch buffer must hold
  size_t scratch_bytes() const
  {
    const size_t a = placed_scratch_bytes(kPlacedSlab), b = lists_bytes();
    return (a > b ? a : b) + checksum_bytes(kPlacedSlab);
  }
  // The manager's own scratch is as large as the calls so far needed (a buffer of a few chunks does not
  // pay for the lists of a full pass); the caller's is scratch_bytes() by contract.
  size_t own_capacity = 0;
  uint8_t* ensure_scratch(size_t need)
  {
    if (scratch && !own_scratch)
      return scratch;
    if (!scratch || own_capacity < need) {
      if (scratch)
        (void)hipFree(scratch); // (waits for whatever still uses it)
      scratch = nullptr;
      own_capacity = 0;
      check(hipMalloc((void**)&scratch, need), "hipMalloc(scratch)");
      own_scratch = true;
      own_capacity = need;
    }
    return scratch;
  }

  hipcomp::CompressionConfig configure_compression(size_t decomp_buffer_size) const
  {
    hipcomp::CompressionConfig c(decomp_buffer_size);
    c.num_chunks = (decomp_buffer_size + chunk_bytes - 1) / chunk_bytes;
    c.max_compressed_buffer_size = layout(c.num_chunks).data + c.num_chunks * slot_bytes;
    return c;
  }

  void compress(const uint8_t* decomp_buffer, uint8_t* comp_buffer, const hipcomp::CompressionConfig& cfg)
  {
    if (reinterpret_cast<uintptr_t>(comp_buffer) & 7)
      throw std::runtime_error("compress: the container buffer must be 8-byte aligned");
    const int R = cascaded_opts.num_RLEs, D = cascaded_opts.num_deltas;
    // (what hipcompBatchedCascadedCompressAsync refuses: cascaded_batch.cpp)
    if (codec == Cascaded
        && (R < 0 || D < 0 || R > 255 || D > 255
            || round_up_to(4 + 4 * (size_t)(R + 1), cascaded_elem) + round_up_to((size_t)cascaded_elem * D, 4) > 64))
      throw std::runtime_error("CascadedManager::compress: num_RLEs / num_deltas do not fit the 64-byte chunk metadata");
    const size_t n = cfg.num_chunks;
    const size_t per_pass = n < kPlacedSlab ? (n ? n : 1) : kPlacedSlab;
    uint8_t* const s = ensure_scratch(placed_scratch_bytes(per_pass) + checksum_bytes(per_pass));
    const Layout lay = layout(n);
    const uint8_t** in_ptrs = reinterpret_cast<const uint8_t**>(s);
    size_t* in_bytes = reinterpret_cast<size_t*>(s + per_pass * 8);
    uint32_t* const ticket = reinterpret_cast<uint32_t*>(s + per_pass * 16);
    uint8_t* const slots = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(s + per_pass * 16 + 64) + 15) & ~uintptr_t(15));
    uint8_t* lz4_temp = reinterpret_cast<uint8_t*>(
        (reinterpret_cast<uintptr_t>(slots + placement_slots() * slot_bytes) + 15) & ~uintptr_t(15));
    header_kernel<<<1, 1, 0, stream>>>(comp_buffer, cfg.uncompressed_buffer_size, n, chunk_bytes, (uint32_t)lay.data,
                                       format, format_header, format_header_bytes, cfg.get_status());
    uint8_t* const csum = computes() ? checksum_area(s + placed_scratch_bytes(per_pass)) : nullptr;
    CrcState* const crc_state = reinterpret_cast<CrcState*>(csum);
    if (csum)
      check(crc_launch_reset(crc_state, stream), "compress: checksums");
    for (size_t first = 0; first < n; first += per_pass) {
      const uint32_t count = (uint32_t)(n - first < per_pass ? n - first : per_pass);
      slab_inputs_kernel<<<(count + kBlock - 1) / kBlock, kBlock, 0, stream>>>(
          decomp_buffer, cfg.uncompressed_buffer_size, chunk_bytes, first, count, in_ptrs, in_bytes, ticket);
      Placement place;
      place.slots = slots;
      place.slot_bytes = slot_bytes;
      place.data = comp_buffer + lay.data;
      place.cursor = reinterpret_cast<unsigned long long*>(comp_buffer + offsetof(CommonHeader, comp_data_size));
      place.offsets = reinterpret_cast<unsigned long long*>(comp_buffer + lay.offsets) + first;
      place.align = place_align;
      // sizes go straight into the container's size array
      size_t* sizes = reinterpret_cast<size_t*>(comp_buffer + lay.sizes) + first;
      switch (codec) {
      case LZ4:
        check(lz4_launch_compress(in_ptrs, in_bytes, nullptr, sizes, ht_size, count, lz4_elem, lz4_temp,
                                  lz4_temp_bytes(per_pass), chunk_bytes, lz4_mode_from_environment(), stream, &place),
              "LZ4Manager::compress");
        break;
      case Snappy:
        check(snappy_launch_compress_placed(in_ptrs, in_bytes, sizes, count, ticket, place, stream),
              "SnappyManager::compress");
        break;
      case Cascaded:
        check(cascaded_launch_compress_placed(in_ptrs, in_bytes, sizes, count, (int)cascaded_opts.type, cascaded_elem, R, D,
                                              cascaded_opts.use_bp ? 1 : 0, ticket, place, stream),
              "CascadedManager::compress");
        break;
      }
      if (csum) {
        // the input slices (arithmetic places) and the placed chunks (in chunk-index order by the scan of sizes)
        const uint64_t slice = slice_bytes(cfg.uncompressed_buffer_size, first, count);
        CrcChunks in;
        in.ptrs = in_ptrs;
        in.lens = in_bytes;
        in.count = count;
        CrcTarget in_t;
        in_t.values = reinterpret_cast<uint32_t*>(comp_buffer + lay.decomp_checksums) + first;
        in_t.stride = chunk_bytes;
        in_t.pass_bytes = slice;
        in_t.pass_word = &crc_state->decomp_pass;
        in_t.flags = &crc_state->flags;
        check(crc_launch_chunks(in, in_t, stream), "compress: checksums");
        CrcChunks out;
        out.base = place.data;
        out.offsets = place.offsets;
        out.lens = sizes;
        out.count = count;
        uint64_t* const work = reinterpret_cast<uint64_t*>(csum + 64);
        check(crc_launch_scan(out, work, crc_state, stream), "compress: checksums");
        CrcTarget out_t;
        out_t.values = reinterpret_cast<uint32_t*>(comp_buffer + lay.comp_checksums) + first;
        out_t.before = work;
        out_t.pass_bytes_dev = &crc_state->comp_pass_bytes;
        out_t.pass_word = &crc_state->comp_pass;
        out_t.flags = &crc_state->flags;
        check(crc_launch_chunks(out, out_t, stream), "compress: checksums");
        check(crc_launch_fold(crc_state, slice, stream), "compress: checksums");
      }
    }
    if (csum)
      check(crc_launch_finish_compress(
                reinterpret_cast<uint32_t*>(comp_buffer + offsetof(CommonHeader, full_comp_buffer_checksum)),
                reinterpret_cast<uint32_t*>(comp_buffer + offsetof(CommonHeader, decomp_buffer_checksum)),
                reinterpret_cast<bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_comp_buffer_checksums)),
                reinterpret_cast<bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_decomp_buffer_checksums)),
                crc_state, stream),
            "compress: checksums");
    check(hipGetLastError(), "compress kernels");
  }

  const CommonHeader& read_header(const uint8_t* comp_buffer)
  {
    check(hipMemcpyAsync(header_host, comp_buffer, sizeof(CommonHeader), hipMemcpyDeviceToHost, stream), "read header");
    check(hipStreamSynchronize(stream), "read header");
    return *header_host;
  }

  // A header that contradicts this manager (another format or chunk size, a chunk count that
  // is not that of its own sizes, data that does not start behind its own tables) configures
  // nothing: status hipcompErrorCannotDecompress, zero bytes, zero chunks -- decompress() then
  // launches nothing.
  bool header_fits(const CommonHeader& h) const
  {
    if (h.format != format || h.uncomp_chunk_size != chunk_bytes || chunk_bytes == 0)
      return false;
    const uint64_t want_chunks = (h.decomp_data_size + chunk_bytes - 1) / chunk_bytes;
    if (h.num_chunks != want_chunks || want_chunks > 0xFFFFFFFFull)
      return false;
    return h.comp_data_offset == layout((size_t)h.num_chunks).data;
  }

  hipcomp::DecompressionConfig configure_decompression(const uint8_t* comp_buffer)
  {
    hipcomp::DecompressionConfig d;
    const CommonHeader& h = read_header(comp_buffer);
    if (!header_fits(h)) {
      *d.get_status() = hipcompErrorCannotDecompress;
      d.decomp_data_size = 0;
      d.num_chunks = 0;
      return d;
    }
    d.decomp_data_size = (size_t)h.decomp_data_size;
    d.num_chunks = (uint32_t)h.num_chunks;
    return d;
  }

  void decompress(uint8_t* decomp_buffer, const uint8_t* comp_buffer, const hipcomp::DecompressionConfig& cfg)
  {
    uint8_t* const s = ensure_scratch(lists_bytes() + checksum_bytes(slab));
    const size_t n = cfg.num_chunks;
    const Layout lay = layout(n);
    const uint8_t** comp_ptrs = reinterpret_cast<const uint8_t**>(s);
    size_t* caps = reinterpret_cast<size_t*>(s + (size_t)slab * 8);
    uint8_t** out_ptrs = reinterpret_cast<uint8_t**>(s + (size_t)slab * 16);
    size_t* actual = reinterpret_cast<size_t*>(s + (size_t)slab * 24);
    hipcompStatus_t* statuses = reinterpret_cast<hipcompStatus_t*>(s + (size_t)slab * 40);
    // (a configuration refused by configure_decompression: nothing to do, its status stands)
    if (n == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() == hipcompErrorCannotDecompress)
      return;
    set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompSuccess);
    // the checksums: read exactly what the decoder is given (comp_ptrs, sizes) and what it wrote (out_ptrs,
    // actual), and only where the container's flags (read on the device) say there are values to compare with
    uint8_t* const csum = verifies() ? checksum_area(s + lists_bytes()) : nullptr;
    CrcState* const crc_state = reinterpret_cast<CrcState*>(csum);
    const bool* const comp_flag =
        reinterpret_cast<const bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_comp_buffer_checksums));
    const bool* const decomp_flag =
        reinterpret_cast<const bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_decomp_buffer_checksums));
    if (csum)
      check(crc_launch_reset(crc_state, stream), "decompress: checksums");
    for (size_t first = 0; first < n; first += slab) {
      const uint32_t count = (uint32_t)(n - first < slab ? n - first : slab);
      slab_streams_kernel<<<(count + kBlock - 1) / kBlock, kBlock, 0, stream>>>(
          comp_buffer, lay.offsets, decomp_buffer, cfg.decomp_data_size, chunk_bytes, first, count, n, format, lay.data,
          comp_ptrs, out_ptrs, caps, cfg.get_status());
      const size_t* sizes = reinterpret_cast<const size_t*>(comp_buffer + lay.sizes) + first;
      switch (codec) {
      case LZ4:
        // (the 64 spare bytes behind the chunk lists hold the decoder's chunk ticket counter)
        check(lz4_launch_decompress(comp_ptrs, sizes, caps, count, out_ptrs, actual, statuses, true, stream,
                                    s + (size_t)slab * 44, 64),
              "LZ4Manager::decompress");
        break;
      case Snappy:
        if (hipcompBatchedSnappyDecompressAsync(reinterpret_cast<const void* const*>(comp_ptrs), sizes, caps, actual, count,
                                                nullptr, 0, reinterpret_cast<void* const*>(out_ptrs), statuses, stream)
            != hipcompSuccess)
          throw std::runtime_error("SnappyManager::decompress: batched decompress failed");
        break;
      case Cascaded:
        if (hipcompBatchedCascadedDecompressAsync(reinterpret_cast<const void* const*>(comp_ptrs), sizes, caps, actual,
                                                  count, nullptr, 0, reinterpret_cast<void* const*>(out_ptrs), statuses,
                                                  stream)
            != hipcompSuccess)
          throw std::runtime_error("CascadedManager::decompress: batched decompress failed");
        break;
      }
      slab_verdict_kernel<<<(count + kBlock - 1) / kBlock, kBlock, 0, stream>>>(statuses, actual, caps, count,
                                                                                  cfg.get_status());
      if (csum) {
        const uint64_t slice = slice_bytes(cfg.decomp_data_size, first, count);
        CrcChunks in;
        in.ptrs = comp_ptrs;
        in.lens = sizes;
        in.caps = caps;
        in.count = count;
        uint64_t* const work = reinterpret_cast<uint64_t*>(csum + 64);
        check(crc_launch_scan(in, work, crc_state, stream), "decompress: checksums");
        CrcTarget in_t;
        in_t.stored = reinterpret_cast<const uint32_t*>(comp_buffer + lay.comp_checksums) + first;
        in_t.present = comp_flag;
        in_t.before = work;
        in_t.pass_bytes_dev = &crc_state->comp_pass_bytes;
        in_t.pass_word = &crc_state->comp_pass;
        in_t.flags = &crc_state->flags;
        check(crc_launch_chunks(in, in_t, stream), "decompress: checksums");
        CrcChunks out;
        out.ptrs = out_ptrs;
        out.lens = actual;
        out.caps = caps;
        out.clamp_to_caps = true;
        out.count = count;
        CrcTarget out_t;
        out_t.stored = reinterpret_cast<const uint32_t*>(comp_buffer + lay.decomp_checksums) + first;
        out_t.present = decomp_flag;
        out_t.stride = chunk_bytes;
        out_t.pass_bytes = slice;
        out_t.pass_word = &crc_state->decomp_pass;
        out_t.flags = &crc_state->flags;
        check(crc_launch_chunks(out, out_t, stream), "decompress: checksums");
        check(crc_launch_fold(crc_state, slice, stream), "decompress: checksums");
      }
    }
    if (csum)
      check(crc_launch_finish_decompress(
                reinterpret_cast<const uint32_t*>(comp_buffer + offsetof(CommonHeader, full_comp_buffer_checksum)),
                reinterpret_cast<const uint32_t*>(comp_buffer + offsetof(CommonHeader, decomp_buffer_checksum)),
                comp_flag, decomp_flag, crc_state, policy == hipcomp::ComputeAndVerify, cfg.get_status(), stream),
            "decompress: checksums");
    check(hipGetLastError(), "decompress kernels");
  }

  // ---- a ranged read: bytes [first_byte, first_byte + num_bytes) of the buffer into out[0, num_bytes) ----
  // The plan is range_plan.hpp's.  Only the chunks the range touches are listed, decoded and (under a verifying
  // policy) checked; a chunk wholly inside the range is decoded straight into out, an edge chunk whole into a
  // scratch slot from which range_slices_kernel moves the wanted span.  The scratch of such a call, carved out of
  // what scratch_bytes() promises (the compress slots and lists lie idle meanwhile): the slots (16-byte aligned,
  // range_slot_stride() each: 2 of them, or one per chunk of a pass where the Cascaded decoder's alignment
  // contract makes every chunk an edge chunk), the pass's chunk lists and the LZ4 decoder's 64 bytes, the CrcState.
  size_t range_slot_stride() const { return (chunk_bytes + 15) & ~size_t(15); }
  static constexpr size_t kRangeFixedBytes = 16 + 64 + 16 + 16 + 64; // alignment, ticket words, alignment x 2, CrcState
  // what the manager's own scratch holds for ranged reads (a constant: no allocation after the first call)
  size_t range_own_bytes() const
  {
    const size_t want = kRangeFixedBytes + (size_t)slab * 44 + (codec == Cascaded ? 1024 : 2) * range_slot_stride();
    const size_t all = scratch_bytes();
    return want < all ? want : all;
  }

  void decompress_range(uint8_t* out, const uint8_t* comp_buffer, const hipcomp::DecompressionConfig& cfg,
                        size_t first_byte, size_t num_bytes)
  {
    // (a configuration refused by configure_decompression: nothing to do, its status stands)
    if (cfg.num_chunks == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() == hipcompErrorCannotDecompress)
      return;
    const size_t stride = range_slot_stride();
    const size_t room = scratch && !own_scratch ? scratch_bytes() : range_own_bytes();
    // chunks per pass with two slots, and with a slot per chunk
    const size_t fixed = kRangeFixedBytes;
    size_t two = room > fixed + 2 * stride ? (room - fixed - 2 * stride) / 44 : 0;
    size_t each = room > fixed ? (room - fixed) / (stride + 44) : 0;
    two = two < slab ? two : slab;
    each = each < two ? each : two;
    if (two < 2)
      throw std::runtime_error("decompress_range: the scratch space does not hold two chunks of this size");
    const uint32_t elem = codec == Cascaded ? (uint32_t)cascaded_elem : 1u;
    // (hipcomp/cascaded.h: buffers 4-byte aligned and aligned to the element type)
    const uint32_t align = codec == Cascaded ? (elem > 4 ? elem : 4u) : 1u;
    range::Plan plan;
    if (!range::range_plan(plan, cfg.decomp_data_size, chunk_bytes, first_byte, num_bytes, (uint32_t)two,
                           (uint32_t)(each < 2 ? 2 : each), align, (uint32_t)(reinterpret_cast<uintptr_t>(out) % align),
                           elem)) {
      set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompErrorInvalidValue);
      check(hipGetLastError(), "decompress_range kernels");
      return;
    }
    set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompSuccess);
    if (plan.chunks == 0) {
      check(hipGetLastError(), "decompress_range kernels");
      return;
    }
    uint8_t* const s = ensure_scratch(room);
    const size_t n = cfg.num_chunks;
    const Layout lay = layout(n);
    const size_t per_pass = plan.chunks < plan.per_pass ? (size_t)plan.chunks : plan.per_pass;
    RangeSlots slots;
    slots.base = checksum_area(s);
    slots.stride = stride;
    uint8_t* const lists = slots.base + (plan.all_edge ? per_pass : 2) * stride;
    const uint8_t** comp_ptrs = reinterpret_cast<const uint8_t**>(lists);
    size_t* caps = reinterpret_cast<size_t*>(lists + per_pass * 8);
    uint8_t** out_ptrs = reinterpret_cast<uint8_t**>(lists + per_pass * 16);
    size_t* actual = reinterpret_cast<size_t*>(lists + per_pass * 24);
    hipcompStatus_t* statuses = reinterpret_cast<hipcompStatus_t*>(lists + per_pass * 32);
    uint8_t* const ticket = checksum_area(lists + per_pass * 36); // (the LZ4 decoder's chunk ticket counter: 64 bytes)
    CrcState* const crc_state = verifies() ? reinterpret_cast<CrcState*>(checksum_area(ticket + 64)) : nullptr;
    const bool* const comp_flag =
        reinterpret_cast<const bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_comp_buffer_checksums));
    const bool* const decomp_flag =
        reinterpret_cast<const bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_decomp_buffer_checksums));
    if (crc_state)
      check(crc_launch_reset(crc_state, stream), "decompress_range: checksums");
    RangeContainer rc;
    rc.container = comp_buffer;
    rc.offsets_at = lay.offsets;
    rc.data_at = lay.data;
    rc.num_chunks = n;
    rc.format = format;
    for (uint64_t k = 0; k < plan.passes; ++k) {
      const uint64_t first = range::range_pass_first(plan, k);
      const uint32_t count = range::range_pass_count(plan, k);
      check(range_launch_list(rc, plan, first, count, out, slots, comp_ptrs, out_ptrs, caps, cfg.get_status(), stream),
            "decompress_range: chunk list");
      const size_t* sizes = reinterpret_cast<const size_t*>(comp_buffer + lay.sizes) + first;
      switch (codec) {
      case LZ4:
        check(lz4_launch_decompress(comp_ptrs, sizes, caps, count, out_ptrs, actual, statuses, true, stream, ticket, 64),
              "LZ4Manager::decompress_range");
        break;
      case Snappy:
        if (hipcompBatchedSnappyDecompressAsync(reinterpret_cast<const void* const*>(comp_ptrs), sizes, caps, actual, count,
                                                nullptr, 0, reinterpret_cast<void* const*>(out_ptrs), statuses, stream)
            != hipcompSuccess)
          throw std::runtime_error("SnappyManager::decompress_range: batched decompress failed");
        break;
      case Cascaded:
        if (hipcompBatchedCascadedDecompressAsync(reinterpret_cast<const void* const*>(comp_ptrs), sizes, caps, actual,
                                                  count, nullptr, 0, reinterpret_cast<void* const*>(out_ptrs), statuses,
                                                  stream)
            != hipcompSuccess)
          throw std::runtime_error("CascadedManager::decompress_range: batched decompress failed");
        break;
      }
      slab_verdict_kernel<<<(count + kBlock - 1) / kBlock, kBlock, 0, stream>>>(statuses, actual, caps, count,
                                                                                  cfg.get_status());
      if (crc_state) {
        // per chunk only: the pass words the CRC kernel also keeps (for the full-buffer checksums, which a partial
        // read cannot check) are not looked at, so no scan of the sizes and no fold
        CrcChunks in;
        in.ptrs = comp_ptrs;
        in.lens = sizes;
        in.caps = caps;
        in.count = count;
        CrcTarget in_t;
        in_t.stored = reinterpret_cast<const uint32_t*>(comp_buffer + lay.comp_checksums) + first;
        in_t.present = comp_flag;
        in_t.pass_bytes = slot_bytes;
        in_t.pass_word = &crc_state->comp_pass;
        in_t.flags = &crc_state->flags;
        check(crc_launch_chunks(in, in_t, stream), "decompress_range: checksums");
        CrcChunks dec;
        dec.ptrs = out_ptrs;
        dec.lens = actual;
        dec.caps = caps;
        dec.clamp_to_caps = true;
        dec.count = count;
        CrcTarget dec_t;
        dec_t.stored = reinterpret_cast<const uint32_t*>(comp_buffer + lay.decomp_checksums) + first;
        dec_t.present = decomp_flag;
        dec_t.stride = chunk_bytes;
        dec_t.pass_bytes = (uint64_t)count * chunk_bytes;
        dec_t.pass_word = &crc_state->decomp_pass;
        dec_t.flags = &crc_state->flags;
        check(crc_launch_chunks(dec, dec_t, stream), "decompress_range: checksums");
      }
      // (where only the range's ends are edge chunks, they are in the first and in the last pass)
      if (plan.all_edge || k == 0 || k + 1 == plan.passes)
        check(range_launch_slices(plan, first, count, out, slots, statuses, actual, caps, stream),
              "decompress_range: slices");
    }
    if (crc_state)
      check(range_launch_finish(comp_flag, decomp_flag, crc_state, policy == hipcomp::ComputeAndVerify, cfg.get_status(),
                                stream),
            "decompress_range: checksums");
    check(hipGetLastError(), "decompress_range kernels");
  }

  // ---- many ranges in one call: range r of the buffer into out[off[r], off[r] + num[r]) ----
  // The arithmetic is gather_plan.hpp's, the kernels gather_kernels.hip's.  The ranges stay on the device: a plan
  // (check and scan, mark, rank) decides there whether the call is refused and numbers the chunks some range
  // touches; the host fetches four words of it -- the call's one synchronisation -- and enqueues the passes.  A pass
  // decodes up to S touched chunks whole, each once, into a scratch slot of its own (list, batched decoder,
  // verdict, checksums: as decompress_range does for its edge chunks) and the copy kernels hand every range its
  // pieces.  The scratch, carved out of what scratch_bytes() promises: the head, the LZ4 decoder's ticket words,
  // the CrcState, the call's tables, S slots, the lists of S chunks.
  static constexpr size_t kRangesOwnSlots = 1024; // what the manager's own scratch holds (the caller's: what fits)
  hipcomp::RangesStats ranges_stats = {};
  GatherHead* ranges_head_host = nullptr; // pinned
  size_t ranges_room(size_t tables) const
  {
    if (scratch && !own_scratch)
      return scratch_bytes();
    const size_t want = (size_t)gather::room_of(kRangesOwnSlots, range_slot_stride(), tables), all = scratch_bytes();
    return want < all ? want : all;
  }
  size_t ranges_pass_chunks() const
  {
    return (size_t)gather::slots_of(ranges_room(0), range_slot_stride(), 0, kPlacedSlab);
  }

  void decompress_ranges(uint8_t* out, size_t out_bytes, const uint8_t* comp_buffer, const hipcomp::DecompressionConfig& cfg,
                         const size_t* device_first_bytes, const size_t* device_num_bytes, size_t num_ranges,
                         size_t* device_out_offsets)
  {
    // (a configuration refused by configure_decompression: nothing to do, its status stands)
    if (cfg.num_chunks == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() == hipcompErrorCannotDecompress)
      return;
    ranges_stats = hipcomp::RangesStats();
    if (num_ranges == 0) {
      *cfg.get_status() = hipcompSuccess;
      return;
    }
    if (num_ranges >= 0xFFFFFFFFull)
      throw std::runtime_error("decompress_ranges: more than 2^32 - 2 ranges");
    const size_t stride = range_slot_stride();
    // (the bitmap has a bit per chunk the configured size has, whatever num_chunks says: a range inside
    // decomp_data_size stays inside it; a num_chunks that differs fails the header test)
    // (at least one word of it, for a buffer of no bytes and ranges of none)
    const uint64_t whole_chunks = ((uint64_t)cfg.decomp_data_size + chunk_bytes - 1) / chunk_bytes;
    const uint64_t bitmap_chunks = whole_chunks ? whole_chunks : 1;
    const size_t tables = (size_t)gather::table_bytes(num_ranges, bitmap_chunks);
    const size_t room = ranges_room(tables);
    const size_t S = (size_t)gather::slots_of(room, stride, tables, kPlacedSlab);
    if (S < 2)
      throw std::runtime_error("decompress_ranges: the scratch space does not hold the tables and two chunks of this size");
    if (!ranges_head_host)
      check(hipHostMalloc((void**)&ranges_head_host, sizeof(GatherHead), hipHostMallocDefault), "hipHostMalloc(ranges)");
    uint8_t* const s = ensure_scratch(room);
    uint8_t* at = checksum_area(s);
    const auto carve = [&at](size_t bytes) {
      uint8_t* const p = at;
      at += gather::round16(bytes);
      return p;
    };
    GatherCall g;
    g.first = device_first_bytes;
    g.num = device_num_bytes;
    g.ranges = num_ranges;
    g.decomp_bytes = cfg.decomp_data_size;
    g.chunk_bytes = chunk_bytes;
    g.elem = codec == Cascaded ? (uint32_t)cascaded_elem : 1u;
    g.words = gather::bitmap_words(bitmap_chunks);
    g.head = reinterpret_cast<GatherHead*>(carve(64));
    uint8_t* const ticket = carve(64); // (the LZ4 decoder's chunk ticket counter)
    CrcState* const crc_state = reinterpret_cast<CrcState*>(carve(64));
    g.offs = reinterpret_cast<uint64_t*>(carve(8 * (num_ranges + 1)));
    g.long_list = reinterpret_cast<uint32_t*>(carve(4 * num_ranges));
    g.bitmap = reinterpret_cast<uint32_t*>(carve(4 * g.words));
    g.word_rank = reinterpret_cast<uint32_t*>(carve(4 * g.words));
    g.group_rank = reinterpret_cast<uint32_t*>(carve(4 * ((g.words + gather::kRankGroup - 1) / gather::kRankGroup)));
    RangeSlots slots;
    slots.base = carve(S * stride);
    slots.stride = stride;
    GatherLists l;
    l.comp_ptrs = reinterpret_cast<const uint8_t**>(at);
    l.comp_sizes = reinterpret_cast<size_t*>(at + S * 8);
    l.caps = reinterpret_cast<size_t*>(at + S * 16);
    l.out_ptrs = reinterpret_cast<uint8_t**>(at + S * 24);
    l.actual = reinterpret_cast<size_t*>(at + S * 32);
    l.statuses = reinterpret_cast<hipcompStatus_t*>(at + S * 40);
    l.comp_sums = reinterpret_cast<uint32_t*>(at + S * 44);
    l.decomp_sums = reinterpret_cast<uint32_t*>(at + S * 48);
    const size_t n = cfg.num_chunks;
    const Layout lay = layout(n);
    RangeContainer rc;
    rc.container = comp_buffer;
    rc.offsets_at = lay.offsets;
    rc.data_at = lay.data;
    rc.num_chunks = n;
    rc.format = format;
    check(gather_launch_plan(g, rc, out_bytes, device_out_offsets, cfg.get_status(), stream), "decompress_ranges: plan");
    check(hipMemcpyAsync(ranges_head_host, g.head, sizeof(GatherHead), hipMemcpyDeviceToHost, stream),
          "decompress_ranges: plan");
    check(hipStreamSynchronize(stream), "decompress_ranges: plan");
    const GatherHead head = *ranges_head_host;
    ranges_stats.ranges = num_ranges;
    ranges_stats.total_bytes = (size_t)head.total_bytes;
    if (head.refused || head.header_bad || head.touched == 0)
      return;
    const uint64_t passes = gather::passes_of(head.touched, S);
    ranges_stats.touched_chunks = head.touched;
    ranges_stats.passes = (size_t)passes;
    const bool* const comp_flag =
        reinterpret_cast<const bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_comp_buffer_checksums));
    const bool* const decomp_flag =
        reinterpret_cast<const bool*>(comp_buffer + offsetof(CommonHeader, include_per_chunk_decomp_buffer_checksums));
    if (verifies())
      check(crc_launch_reset(crc_state, stream), "decompress_ranges: checksums");
    for (uint64_t k = 0; k < passes; ++k) {
      const uint32_t count = (uint32_t)gather::pass_count(head.touched, S, k);
      check(gather_launch_list(g, rc, lay.sizes, lay.comp_checksums, lay.decomp_checksums, S, k, count, slots, l,
                               cfg.get_status(), stream),
            "decompress_ranges: chunk list");
      switch (codec) {
      case LZ4:
        check(lz4_launch_decompress(l.comp_ptrs, l.comp_sizes, l.caps, count, l.out_ptrs, l.actual, l.statuses, true, stream,
                                    ticket, 64),
              "LZ4Manager::decompress_ranges");
        break;
      case Snappy:
        if (hipcompBatchedSnappyDecompressAsync(reinterpret_cast<const void* const*>(l.comp_ptrs), l.comp_sizes, l.caps,
                                                l.actual, count, nullptr, 0, reinterpret_cast<void* const*>(l.out_ptrs),
                                                l.statuses, stream)
            != hipcompSuccess)
          throw std::runtime_error("SnappyManager::decompress_ranges: batched decompress failed");
        break;
      case Cascaded:
        if (hipcompBatchedCascadedDecompressAsync(reinterpret_cast<const void* const*>(l.comp_ptrs), l.comp_sizes, l.caps,
                                                  l.actual, count, nullptr, 0, reinterpret_cast<void* const*>(l.out_ptrs),
                                                  l.statuses, stream)
            != hipcompSuccess)
          throw std::runtime_error("CascadedManager::decompress_ranges: batched decompress failed");
        break;
      }
      slab_verdict_kernel<<<(count + kBlock - 1) / kBlock, kBlock, 0, stream>>>(l.statuses, l.actual, l.caps, count,
                                                                                  cfg.get_status());
      if (verifies()) {
        // per chunk only, as in decompress_range; the stored values are the pass's gathered lists
        CrcChunks in;
        in.ptrs = l.comp_ptrs;
        in.lens = l.comp_sizes;
        in.caps = l.caps;
        in.count = count;
        CrcTarget in_t;
        in_t.stored = l.comp_sums;
        in_t.present = comp_flag;
        in_t.pass_bytes = slot_bytes;
        in_t.pass_word = &crc_state->comp_pass;
        in_t.flags = &crc_state->flags;
        check(crc_launch_chunks(in, in_t, stream), "decompress_ranges: checksums");
        CrcChunks dec;
        dec.ptrs = l.out_ptrs;
        dec.lens = l.actual;
        dec.caps = l.caps;
        dec.clamp_to_caps = true;
        dec.count = count;
        CrcTarget dec_t;
        dec_t.stored = l.decomp_sums;
        dec_t.present = decomp_flag;
        dec_t.stride = chunk_bytes;
        dec_t.pass_bytes = (uint64_t)count * chunk_bytes;
        dec_t.pass_word = &crc_state->decomp_pass;
        dec_t.flags = &crc_state->flags;
        check(crc_launch_chunks(dec, dec_t, stream), "decompress_ranges: checksums");
      }
      check(gather_launch_copy(g, out, S, k, count, head.long_ranges, head.long_span, slots, l, stream),
            "decompress_ranges: copy");
    }
    if (verifies())
      check(range_launch_finish(comp_flag, decomp_flag, crc_state, policy == hipcomp::ComputeAndVerify, cfg.get_status(),
                                stream),
            "decompress_ranges: checksums");
    check(hipGetLastError(), "decompress_ranges kernels");
  }

  // ---- LZ4 frames (hipcomp/lz4.hpp; the format: lz4_frame.hpp; the kernels: lz4_frame_launch.hpp) ----
  // Both directions work in passes of as many blocks as fit the scratch space scratch_bytes() promises, like
  // decompress_range; the manager's own scratch is as large as the call at hand needs, up to that.
  // Writing, a pass of P chunks: the frame cursor (16 bytes), six lists (44 bytes per chunk), a slot per chunk for
  // the batched encoder (unplaced: the frame wants the blocks in chunk order and the stored ones from the input),
  // the encoder's temp space.
  size_t frame_write_bytes(size_t P) const { return 16 + 16 + 44 * P + 16 + P * slot_bytes + 16 + lz4_temp_bytes(P); }
  size_t frame_write_pass(size_t chunks) const
  {
    const size_t room = scratch_bytes();
    size_t P = chunks < kPlacedSlab ? (chunks ? chunks : 1) : kPlacedSlab;
    if (frame_write_bytes(P) <= room)
      return P;
    size_t lo = 1; // (fits: scratch_bytes() holds a slot per resident wave and a full pass's lists)
    while (lo < P) {
      const size_t mid = lo + (P - lo + 1) / 2;
      if (frame_write_bytes(mid) <= room)
        lo = mid;
      else
        P = mid - 1;
    }
    return lo;
  }
  // Reading, a pass of P blocks: the walk's state (128 bytes), the batched decoder's ticket words (64), the indexed
  // read's state (lz4_frame_index_launch.hpp), the entry lists.  The state fills the 2048 bytes to the last one
  // (128 + 64 + 1856): a larger IndexState needs a larger kFrameReadLists.  The required scratch is what it was, so
  // a pass of every frame read, indexed or not, holds 1856 / kReadEntryBytes = 22 entries fewer than before the index;
  // that matters only where the scratch and not kPlacedSlab bounds the pass (chunks of a few bytes).
  static constexpr size_t kFrameReadLists = 2048;
  static constexpr size_t kFrameReadFixed = 16 + kFrameReadLists;
  static_assert(128 + 64 + sizeof(lz4f::IndexState) <= kFrameReadLists, "the indexed read's state does not fit");
  static lz4f::IndexState* frame_index_state(uint8_t* s) { return reinterpret_cast<lz4f::IndexState*>(s + 128 + 64); }
  size_t frame_read_bytes(size_t P) const { return kFrameReadFixed + lz4f::kReadEntryBytes * P; }
  size_t frame_read_pass(size_t blocks) const
  {
    size_t P = (scratch_bytes() - kFrameReadFixed) / lz4f::kReadEntryBytes;
    P = P < kPlacedSlab ? P : kPlacedSlab;
    return blocks < P ? (blocks ? blocks : 1) : P;
  }
  static lz4f::ReadLists frame_read_lists(uint8_t* at, size_t P)
  {
    lz4f::ReadLists l;
    l.comp_ptrs = reinterpret_cast<const uint8_t**>(at);
    l.comp_bytes = reinterpret_cast<size_t*>(at + 8 * P);
    l.batch_bytes = reinterpret_cast<size_t*>(at + 16 * P);
    l.sizes = reinterpret_cast<size_t*>(at + 24 * P);
    l.out_ptrs = reinterpret_cast<uint8_t**>(at + 32 * P);
    l.caps = reinterpret_cast<size_t*>(at + 40 * P);
    l.batch_caps = reinterpret_cast<size_t*>(at + 48 * P);
    l.actual = reinterpret_cast<size_t*>(at + 56 * P);
    l.aux = reinterpret_cast<uint64_t*>(at + 64 * P);
    l.flags = reinterpret_cast<uint32_t*>(at + 72 * P);
    l.head = reinterpret_cast<int32_t*>(at + 76 * P);
    l.statuses = reinterpret_cast<hipcompStatus_t*>(at + 80 * P);
    return l;
  }

  // index: the frame gets its block index in front of it (lz4_frame_index.hpp), 44 + 4 * num_chunks bytes more
  hipcomp::CompressionConfig configure_frame_compression(size_t decomp_buffer_size, bool index = false) const
  {
    hipcomp::CompressionConfig c(decomp_buffer_size);
    if (lz4f::code_for_chunk(chunk_bytes) == 0) { // no block maximum of the format holds a chunk
      *c.get_status() = hipcompErrorInvalidValue;
      return c;
    }
    c.num_chunks = (decomp_buffer_size + chunk_bytes - 1) / chunk_bytes;
    // (a frame of 2^32 blocks or more cannot be indexed: its N is a u32)
    if (index && c.num_chunks > 0xFFFFFFFFull) {
      *c.get_status() = hipcompErrorInvalidValue;
      c.num_chunks = 0;
      return c;
    }
    c.max_compressed_buffer_size = (size_t)lz4f::frame_bound(c.num_chunks, chunk_bytes, computes())
                                   + (index ? (size_t)lz4f::index_bytes(c.num_chunks) : 0);
    return c;
  }

  // index: the room of the index is left in front of the frame, its words are written pass by pass from the lists
  // write_blocks_kernel reads, its hash once they all stand
  void compress_frame(const uint8_t* decomp_buffer, uint8_t* const buffer, const hipcomp::CompressionConfig& cfg,
                      size_t* frame_bytes, bool index = false)
  {
    if (reinterpret_cast<uintptr_t>(frame_bytes) & 7)
      throw std::runtime_error("compress_frame: frame_bytes must be 8-byte aligned");
    const uint32_t code = lz4f::code_for_chunk(chunk_bytes);
    if (code == 0 || (index && cfg.num_chunks > 0xFFFFFFFFull)) {
      set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompErrorInvalidValue);
      check(lz4f::launch_set_size(frame_bytes, 0, stream), "compress_frame");
      return;
    }
    const size_t n = cfg.num_chunks;
    uint8_t* const frame = buffer + (index ? (size_t)lz4f::index_bytes(n) : 0);
    const size_t P = frame_write_pass(n);
    uint8_t* const s = checksum_area(ensure_scratch(frame_write_bytes(P)));
    unsigned long long* const cursor = reinterpret_cast<unsigned long long*>(s);
    uint8_t* const lists = s + 16;
    lz4f::WriteLists l;
    l.in_ptrs = reinterpret_cast<const uint8_t**>(lists);
    l.in_bytes = reinterpret_cast<size_t*>(lists + 8 * P);
    l.slots = reinterpret_cast<uint8_t**>(lists + 16 * P);
    l.stream_bytes = reinterpret_cast<size_t*>(lists + 24 * P);
    l.offsets = reinterpret_cast<uint64_t*>(lists + 32 * P);
    l.sums = reinterpret_cast<uint32_t*>(lists + 40 * P);
    uint8_t* const slots = checksum_area(lists + 44 * P);
    uint8_t* const temp = checksum_area(slots + P * slot_bytes);
    const bool sums = computes();
    set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompSuccess);
    if (index)
      check(lz4f::launch_index_write_fields(buffer, (uint32_t)n, (uint32_t)chunk_bytes, cfg.uncompressed_buffer_size, sums,
                                            stream),
            "compress_frame: index");
    check(lz4f::launch_write_header(frame, cfg.uncompressed_buffer_size, code, sums, cursor, stream), "compress_frame: header");
    for (size_t first = 0; first < n; first += P) {
      const uint32_t count = (uint32_t)(n - first < P ? n - first : P);
      check(lz4f::launch_write_lists(decomp_buffer, cfg.uncompressed_buffer_size, chunk_bytes, first, count, slots, slot_bytes,
                                     l, stream),
            "compress_frame: chunk lists");
      check(lz4_launch_compress(l.in_ptrs, l.in_bytes, l.slots, l.stream_bytes, ht_size, count, lz4_elem, temp,
                                lz4_temp_bytes(P), chunk_bytes, lz4_mode_from_environment(), stream, nullptr),
            "LZ4Manager::compress_frame");
      check(lz4f::launch_write_scan(l, count, sums, cursor, stream), "compress_frame: scan");
      if (sums)
        check(lz4f::launch_write_sums(l, count, stream), "compress_frame: block checksums");
      check(lz4f::launch_write_blocks(frame, l, count, chunk_bytes, sums, stream), "compress_frame: blocks");
      if (index)
        check(lz4f::launch_index_write_words(buffer, l, first, count, stream), "compress_frame: index");
    }
    check(lz4f::launch_write_end(frame, cursor, frame_bytes, stream), "compress_frame: end mark");
    if (index)
      check(lz4f::launch_index_write_end(buffer, (uint32_t)n, frame_bytes, stream), "compress_frame: index");
    check(hipGetLastError(), "compress_frame kernels");
  }

  // the entries of one pass: the walk, the sizes (the batched decoder's parse-only pass; the token walk for linked
  // frames), the scan that places them
  void frame_pass_lists(const uint8_t* frames, size_t frames_bytes, lz4f::ReadState* st, const lz4f::ReadLists& l,
                        uint32_t count, void* ticket, uint8_t* out, uint64_t out_bytes, lz4f::IndexState* ix = nullptr)
  {
    check(lz4f::launch_read_walk(frames, frames_bytes, st, &l, count, verifies(), stream, ix ? &ix->skip : nullptr),
          "frame: walk");
    check(lz4f::launch_read_linked_sizes(l, st, count, stream), "frame: sizes");
    check(lz4_launch_decompress(l.comp_ptrs, l.batch_bytes, nullptr, count, nullptr, l.actual, nullptr, false, stream,
                                ticket, 64),
          "frame: sizes");
    check(lz4f::launch_read_scan(l, st, count, out, out_bytes, stream), "frame: scan");
  }

  // What configure_frame_decompression found in front of the frames of the buffer it saw last: decompress_frame
  // does not launch the indexed passes for a buffer that had no index then.  A hint and no more -- the passes
  // themselves decide on the device, whatever the buffer holds by now.
  const uint8_t* hint_frames = nullptr;
  size_t hint_bytes = 0;
  bool hint_indexed = false;
  // the state of the last decompress_frame or decompress_frame_range
  lz4f::ReadState* last_read_state = nullptr;

  // Blocks the chain's walk stepped over in the last decompress_frame or decompress_frame_range (synchronises the
  // stream): ReadState::walked, which the walk alone adds to, block by block.
  size_t frame_walked_blocks()
  {
    if (!last_read_state)
      return 0;
    lz4f::ReadState h;
    check(hipMemcpyAsync(&h, last_read_state, sizeof(h), hipMemcpyDeviceToHost, stream), "frame_walked_blocks");
    check(hipStreamSynchronize(stream), "frame_walked_blocks");
    return (size_t)h.walked;
  }

  hipcomp::DecompressionConfig configure_frame_decompression(const uint8_t* frames, size_t frames_bytes)
  {
    hipcomp::DecompressionConfig d;
    uint8_t* s = checksum_area(ensure_scratch(frame_read_bytes(1)));
    lz4f::ReadState* st = reinterpret_cast<lz4f::ReadState*>(s);
    lz4f::ReadState h;
    auto fetch = [&] {
      check(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, stream), "configure_frame_decompression");
      check(hipStreamSynchronize(stream), "configure_frame_decompression");
    };
    // indexed frames and nothing else: the numbers are the indexes', every block tested in its place
    {
      lz4f::IndexState* const ix = frame_index_state(s);
      lz4f::IndexState hx;
      check(lz4f::launch_index_begin(frames, frames_bytes, ix, stream), "configure_frame_decompression: index");
      check(lz4f::launch_index_list(frames, frames_bytes, ix, st, nullptr, 0, nullptr, 0, stream),
            "configure_frame_decompression: index");
      check(hipMemcpyAsync(&hx, ix, offsetof(lz4f::IndexState, frame), hipMemcpyDeviceToHost, stream),
            "configure_frame_decompression");
      check(hipStreamSynchronize(stream), "configure_frame_decompression");
      hint_frames = frames;
      hint_bytes = frames_bytes;
      hint_indexed = hx.ok && hx.listed == hx.blocks;
      if (hint_indexed) {
        d.num_chunks = (uint32_t)hx.blocks;
        d.decomp_data_size = (size_t)hx.content_bytes;
        return d;
      }
    }
    check(lz4f::launch_read_reset(st, stream), "configure_frame_decompression");
    check(lz4f::launch_read_walk(frames, frames_bytes, st, nullptr, 0, false, stream), "configure_frame_decompression");
    fetch();
    if (h.reason != lz4f::kOk) {
      *d.get_status() = (hipcompStatus_t)lz4f::status_of(h.reason);
      return d;
    }
    d.num_chunks = (uint32_t)h.blocks;
    if (h.all_declared) {
      d.decomp_data_size = (size_t)h.declared_sum;
      return d;
    }
    // a frame does not say: the sizes are those the blocks parse to
    const size_t blocks = (size_t)h.blocks, P = frame_read_pass(blocks);
    s = checksum_area(ensure_scratch(frame_read_bytes(P)));
    st = reinterpret_cast<lz4f::ReadState*>(s);
    const lz4f::ReadLists l = frame_read_lists(s + kFrameReadLists, P);
    check(lz4f::launch_read_reset(st, stream), "configure_frame_decompression");
    for (size_t first = 0; first < blocks; first += P) {
      const uint32_t count = (uint32_t)(blocks - first < P ? blocks - first : P);
      frame_pass_lists(frames, frames_bytes, st, l, count, s + 128, nullptr, ~uint64_t(0));
    }
    fetch();
    d.decomp_data_size = (size_t)h.out_cursor;
    return d;
  }

  void decompress_frame(uint8_t* decomp_buffer, const uint8_t* frames, size_t frames_bytes,
                        const hipcomp::DecompressionConfig& cfg)
  {
    // (a configuration refused by configure_frame_decompression: nothing to do, its status stands)
    if (cfg.num_chunks == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() != hipcompSuccess)
      return;
    const size_t blocks = cfg.num_chunks, P = frame_read_pass(blocks);
    uint8_t* const s = checksum_area(ensure_scratch(frame_read_bytes(P)));
    lz4f::ReadState* const st = reinterpret_cast<lz4f::ReadState*>(s);
    void* const ticket = s + 128;
    // (no indexed passes for a buffer that had no index when it was configured: the parent's launches, one for one)
    const bool try_index = !(hint_frames == frames && hint_bytes == frames_bytes && !hint_indexed);
    lz4f::IndexState* const ix = try_index ? frame_index_state(s) : nullptr;
    last_read_state = st;
    const lz4f::ReadLists l = frame_read_lists(s + kFrameReadLists, P);
    check(lz4f::launch_read_reset(st, stream), "decompress_frame");
    // The indexed passes: entries from the index (no walk, no parse-only pass), the batched decoder, the stored
    // blocks, the block checksums.  Whether they held is a word on the device: if so the chain's passes below find
    // nothing to do, if not they start from the reset state and do it all.
    if (try_index) {
      check(lz4f::launch_index_begin(frames, frames_bytes, ix, stream), "decompress_frame: index");
      for (size_t first = 0; first < blocks; first += P) {
        const uint32_t count = (uint32_t)(blocks - first < P ? blocks - first : P);
        check(lz4f::launch_index_list(frames, frames_bytes, ix, st, &l, count, decomp_buffer, cfg.decomp_data_size, stream),
              "decompress_frame: index");
        check(lz4_launch_decompress(l.comp_ptrs, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, true,
                                    stream, ticket, 64),
              "LZ4Manager::decompress_frame");
        check(lz4f::launch_index_verdict(l, st, ix, count, stream), "decompress_frame: index");
        check(lz4f::launch_read_stored(l, st, count, 2 * (uint64_t)(cfg.decomp_data_size / blocks), stream),
              "decompress_frame: stored blocks");
        if (verifies())
          check(lz4f::launch_read_block_sums(l, st, count, stream), "decompress_frame: block checksums");
      }
      check(lz4f::launch_index_end(ix, st, l, (uint32_t)(blocks < P ? blocks : P), frames_bytes, blocks, stream),
            "decompress_frame: index");
    }
    const uint32_t* const skip = ix ? &ix->skip : nullptr;
    for (size_t first = 0; first < blocks; first += P) {
      const uint32_t count = (uint32_t)(blocks - first < P ? blocks - first : P);
      frame_pass_lists(frames, frames_bytes, st, l, count, ticket, decomp_buffer, cfg.decomp_data_size, ix);
      check(lz4_launch_decompress(l.comp_ptrs, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, true,
                                  stream, ticket, 64),
            "LZ4Manager::decompress_frame");
      check(lz4f::launch_read_verdict(l, st, count, stream), "decompress_frame: verdict");
      // (workgroups per stored block by the size of the average block: the sizes themselves are on the device)
      check(lz4f::launch_read_stored(l, st, count, 2 * (uint64_t)(cfg.decomp_data_size / blocks), stream),
            "decompress_frame: stored blocks");
      check(lz4f::launch_read_linked(l, st, count, decomp_buffer, stream), "decompress_frame: linked blocks");
      if (verifies()) {
        check(lz4f::launch_read_block_sums(l, st, count, stream), "decompress_frame: block checksums");
        check(lz4f::launch_read_content_sums(l, st, count, decomp_buffer, stream), "decompress_frame: content checksums");
      }
      check(lz4f::launch_read_pass_end(l, st, decomp_buffer, stream), "decompress_frame");
    }
    // what lies behind the last block (trailers are read with their block; skippable and empty frames here)
    check(lz4f::launch_read_walk(frames, frames_bytes, st, &l, 0, verifies(), stream, skip), "decompress_frame: walk");
    check(lz4f::launch_read_finish(st, blocks, cfg.decomp_data_size, policy == hipcomp::ComputeAndVerify, cfg.get_status(),
                                   stream),
          "decompress_frame");
    check(hipGetLastError(), "decompress_frame kernels");
  }

  // ---- a batch of frames in one call (hipcomp/lz4.hpp, decompress_frames; the arithmetic: lz4_frames_plan.hpp; the
  // kernels: lz4_frames_launch.hpp) ----
  // Every item has a walk's state of its own at the head of the scratch space.  The first walk counts every item's
  // data blocks, a scan numbers them through the batch, and the host reads the totals: the one synchronisation.
  // Then passes of as many blocks as the lists behind the states hold, whatever items they belong to; each is a
  // pass of decompress_frame with the verdicts going to the entries' items.  decode == false: the size query, the
  // passes stop behind the placing scan.
  // The manager's own scratch is grown to the states and kFramesOwnEntries entries; the caller's is scratch_bytes().
  static constexpr size_t kFramesOwnEntries = 65536;
  size_t frames_pass_limit = 0; // (set_frames_pass_entries: tests and measurements bound a pass with it; 0: no bound)
  hipcomp::LZ4FramesStats frames_stats = {};
  void frames_call(const uint8_t* const* item_ptrs, const size_t* item_bytes, uint8_t* const* out_ptrs, const size_t* out_caps,
                   size_t* sizes, hipcompStatus_t* statuses, size_t num_items, lz4fb::Prefix prefix, bool decode, const char* who)
  {
    frames_stats = hipcomp::LZ4FramesStats();
    if (num_items == 0)
      return;
    if (num_items > lz4fb::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (!item_ptrs || !item_bytes || !sizes || (decode && (!out_ptrs || !out_caps || !statuses)))
      throw std::runtime_error(std::string(who) + ": a null array");
    lz4fb::Batch b;
    b.item_ptrs = item_ptrs;
    b.item_bytes = item_bytes;
    b.out_ptrs = decode ? out_ptrs : nullptr;
    b.out_capacities = decode ? out_caps : nullptr;
    b.items = num_items;
    b.prefix = prefix;
    if (!decode && prefix == lz4fb::kArrowLength) { // the prefixes say it
      frames_stats.items = num_items;
      check(lz4fb::launch_prefix_sizes(b, sizes, stream), who);
      return;
    }
    const bool callers = scratch && !own_scratch;
    const size_t own_need = (size_t)lz4fb::scratch_bytes(num_items, kFramesOwnEntries);
    const size_t room = callers ? scratch_bytes() : (own_capacity > own_need ? own_capacity : own_need);
    // (16 bytes of it may go to the alignment of a caller's buffer)
    size_t P = (size_t)lz4fb::pass_entries(room - 16, num_items, kPlacedSlab);
    if (P == 0)
      throw std::runtime_error(std::string(who) + ": the scratch space does not hold the state of the items and two blocks' entries");
    if (frames_pass_limit && frames_pass_limit < P)
      P = frames_pass_limit;
    frames_stats.items = num_items; // (behind everything that throws: a call that threw launched nothing and counts nothing)
    uint8_t* const s = checksum_area(ensure_scratch(room));
    lz4fb::Item* const items = reinterpret_cast<lz4fb::Item*>(s);
    lz4fb::Totals* const totals = reinterpret_cast<lz4fb::Totals*>(s + lz4fb::totals_at(num_items));
    void* const ticket = s + lz4fb::ticket_at(num_items);
    const lz4f::ReadLists l = frame_read_lists(s + lz4fb::lists_at(num_items), P);
    uint32_t* const item_col = reinterpret_cast<uint32_t*>(s + lz4fb::item_column_at(num_items, P));
    check(lz4fb::launch_begin(b, items, !decode, stream), who);
    check(lz4fb::launch_scan_items(items, num_items, totals, stream), who);
    lz4fb::Totals h;
    check(hipMemcpyAsync(&h, totals, sizeof(h), hipMemcpyDeviceToHost, stream), who);
    check(hipStreamSynchronize(stream), who);
    const uint64_t passes = lz4fb::passes_of(h.blocks, P);
    frames_stats.blocks = (size_t)h.blocks;
    frames_stats.passes = (size_t)passes;
    frames_stats.pass_entries = P;
    for (uint64_t k = 0; k < passes; ++k) {
      const uint32_t count = (uint32_t)lz4fb::pass_count(h.blocks, P, k);
      check(lz4fb::launch_list(items, num_items, l, item_col, P, k, decode && verifies(), stream), "frames: walk");
      check(lz4fb::launch_linked_sizes(l, count, stream), "frames: sizes");
      check(lz4_launch_decompress(l.comp_ptrs, l.batch_bytes, nullptr, count, nullptr, l.actual, nullptr, false, stream, ticket,
                                  64),
            "frames: sizes");
      check(lz4fb::launch_place(items, l, item_col, count, k * P, stream), "frames: scan");
      if (!decode)
        continue;
      check(lz4_launch_decompress(l.comp_ptrs, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, true,
                                  stream, ticket, 64),
            "LZ4Manager::decompress_frames");
      check(lz4fb::launch_batched_verdict(items, l, item_col, count, stream), "frames: verdict");
      check(lz4fb::launch_stored(l, count, h.largest, stream), "frames: stored blocks");
      check(lz4fb::launch_linked(items, l, item_col, count, stream), "frames: linked blocks");
      if (verifies()) {
        check(lz4fb::launch_block_sums(items, l, item_col, count, stream), "frames: block checksums");
        check(lz4fb::launch_content_sums(items, l, item_col, count, stream), "frames: content checksums");
      }
      check(lz4fb::launch_pass_end(items, l, item_col, count, stream), "frames: pass end");
    }
    check(lz4fb::launch_finish(items, num_items, verifies(), policy == hipcomp::ComputeAndVerify, sizes,
                               decode ? statuses : nullptr, stream),
          who);
    check(hipGetLastError(), who);
  }

  // ---- the pages of a batch of Parquet column chunks (hipcomp/snappy.hpp, decompress_parquet_pages; the arithmetic
  // and the page rules: parquet_pages_plan.hpp; the kernels and the passes: parquet_pages_launch.hpp) ----
  // What is decided here: the scratch space.  The manager's own is grown to the items' states and kPagesOwnEntries
  // pages' entries; the caller's is scratch_bytes().
  static constexpr size_t kPagesOwnEntries = 65536;
  size_t pages_pass_limit = 0; // (set_parquet_pass_pages: tests and measurements bound a pass with it; 0: no bound)
  hipcomp::ParquetPagesStats pages_stats = {};
  static void pages_batch(pqp::Batch& b, const uint8_t* const* chunk_ptrs, const size_t* chunk_bytes, size_t num_chunks,
                          hipcomp::ParquetCodec codec, const char* who)
  {
    if (num_chunks > pqp::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 chunks");
    if (codec != hipcomp::ParquetCodec::Uncompressed && codec != hipcomp::ParquetCodec::Snappy)
      throw std::runtime_error(std::string(who) + ": unknown ParquetCodec");
    b = pqp::Batch();
    b.chunk_ptrs = chunk_ptrs;
    b.chunk_bytes = chunk_bytes;
    b.items = num_chunks;
    b.codec = codec == hipcomp::ParquetCodec::Snappy ? pqp::kCompressedColumn : pqp::kStoredColumn;
  }
  void pages_sizes(const uint8_t* const* chunk_ptrs, const size_t* chunk_bytes, size_t* num_pages, size_t* sizes,
                   hipcompStatus_t* statuses, size_t num_chunks, hipcomp::ParquetCodec codec)
  {
    const char* const who = "get_parquet_pages_sizes";
    pqp::Batch b;
    pages_batch(b, chunk_ptrs, chunk_bytes, num_chunks, codec, who);
    if (num_chunks == 0)
      return;
    if (!chunk_ptrs || !chunk_bytes || !num_pages || !sizes || !statuses)
      throw std::runtime_error(std::string(who) + ": a null array");
    check(pqp::launch_sizes(b, num_pages, sizes, statuses, stream), who);
  }
  void pages_call(const uint8_t* const* chunk_ptrs, const size_t* chunk_bytes, uint8_t* const* out_ptrs, const size_t* out_caps,
                  size_t* sizes, hipcompStatus_t* statuses, hipcomp::ParquetPageInfo* const* page_ptrs, const size_t* page_caps,
                  size_t* num_pages, size_t num_chunks, hipcomp::ParquetCodec codec)
  {
    const char* const who = "decompress_parquet_pages";
    static_assert(sizeof(hipcomp::ParquetPageInfo) == sizeof(pqp::Page) && alignof(hipcomp::ParquetPageInfo) == alignof(pqp::Page),
                  "ParquetPageInfo is the plan's page record");
    pages_stats = hipcomp::ParquetPagesStats();
    pqp::Batch b;
    pages_batch(b, chunk_ptrs, chunk_bytes, num_chunks, codec, who);
    if (num_chunks == 0)
      return;
    if (!chunk_ptrs || !chunk_bytes || !out_ptrs || !out_caps || !sizes || !statuses || !num_pages || (page_ptrs && !page_caps))
      throw std::runtime_error(std::string(who) + ": a null array");
    b.out_ptrs = out_ptrs;
    b.out_capacities = out_caps;
    b.page_ptrs = reinterpret_cast<pqp::Page* const*>(page_ptrs);
    b.page_capacities = page_caps;
    const bool callers = scratch && !own_scratch;
    const size_t own_need = (size_t)pqp::scratch_bytes(num_chunks, kPagesOwnEntries) + 16;
    const size_t room = callers ? scratch_bytes() : (own_capacity > own_need ? own_capacity : own_need);
    // (16 bytes of it may go to the alignment of a caller's buffer)
    size_t P = (size_t)pqp::pass_entries(room - 16, num_chunks, kPlacedSlab);
    if (P == 0)
      throw std::runtime_error(std::string(who) + ": the scratch space does not hold the state of the chunks and two pages' entries");
    if (pages_pass_limit && pages_pass_limit < P)
      P = pages_pass_limit;
    uint8_t* const s = checksum_area(ensure_scratch(room));
    pqp::Stats found;
    check(pqp::run(b, sizes, statuses, num_pages, s, P, verifies(), policy == hipcomp::ComputeAndVerify, stream, &found), who);
    pages_stats.items = num_chunks;
    pages_stats.pages = (size_t)found.pages;
    pages_stats.passes = (size_t)found.passes;
    pages_stats.pass_pages = P;
  }

  // ---- a batch of Parquet RLE / bit-packed hybrid streams (hipcomp/cascaded.hpp, decode_parquet_hybrid; the
  // arithmetic and the rules: parquet_hybrid_plan.hpp; the kernel: parquet_hybrid_launch.hpp) ----
  // One launch on the manager's stream: no scratch, no synchronisation, nothing of the host's read back.
  void hybrid_call(const uint8_t* const* stream_ptrs, const size_t* stream_bytes, const uint32_t* bit_widths, const size_t* num_values,
                   void* const* out_ptrs, const size_t* out_caps, size_t* consumed, const uint32_t* match_values, size_t* match_counts,
                   hipcompStatus_t* statuses, size_t num_items, hipcomp::ParquetHybridForm form, hipcompType_t out_type)
  {
    const char* const who = "decode_parquet_hybrid";
    static_assert((uint32_t)hipcomp::ParquetHybridForm::Bare == pqh::kBare
                      && (uint32_t)hipcomp::ParquetHybridForm::LengthPrefixed == pqh::kLengthPrefixed
                      && (uint32_t)hipcomp::ParquetHybridForm::WidthPrefixed == pqh::kWidthPrefixed,
                  "ParquetHybridForm is the plan's Form");
    if (num_items > pqh::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (form != hipcomp::ParquetHybridForm::Bare && form != hipcomp::ParquetHybridForm::LengthPrefixed
        && form != hipcomp::ParquetHybridForm::WidthPrefixed)
      throw std::runtime_error(std::string(who) + ": unknown ParquetHybridForm");
    uint32_t element_bytes = 0;
    switch (out_type) {
    case HIPCOMP_TYPE_UCHAR: element_bytes = 1; break;
    case HIPCOMP_TYPE_USHORT: element_bytes = 2; break;
    case HIPCOMP_TYPE_UINT: element_bytes = 4; break;
    default: throw std::runtime_error(std::string(who) + ": the elements are UCHAR, USHORT or UINT");
    }
    if (num_items == 0)
      return;
    if (!stream_ptrs || !stream_bytes || !num_values || !out_ptrs || !out_caps || !statuses
        || (!bit_widths && form != hipcomp::ParquetHybridForm::WidthPrefixed))
      throw std::runtime_error(std::string(who) + ": a null array");
    if ((match_values == nullptr) != (match_counts == nullptr))
      throw std::runtime_error(std::string(who) + ": the match values and the match counts come together");
    pqh::Batch b;
    b.stream_ptrs = stream_ptrs;
    b.stream_bytes = stream_bytes;
    b.bit_widths = bit_widths;
    b.num_values = num_values;
    b.out_ptrs = out_ptrs;
    b.out_capacities = out_caps;
    b.consumed_bytes = consumed;
    b.match_values = match_values;
    b.match_counts = match_counts;
    b.statuses = statuses;
    b.items = num_items;
    b.form = (uint32_t)form;
    check(pqh::launch(b, element_bytes, stream), who);
  }

  // ---- a batch of Parquet DELTA_BINARY_PACKED streams (hipcomp/cascaded.hpp, decode_parquet_delta; the arithmetic and
  // the rules: parquet_delta_plan.hpp; the kernel: parquet_delta_launch.hpp) ----
  // One launch on the manager's stream: no scratch, no synchronisation, nothing of the host's read back.
  void delta_call(const uint8_t* const* stream_ptrs, const size_t* stream_bytes, const size_t* num_values, void* const* out_ptrs,
                  const size_t* out_caps, size_t* value_counts, size_t* consumed, hipcompStatus_t* statuses, size_t num_items,
                  hipcomp::ParquetDeltaOutput output, hipcompType_t out_type)
  {
    const char* const who = "decode_parquet_delta";
    static_assert((uint32_t)hipcomp::ParquetDeltaOutput::Values == pqd::kValues
                      && (uint32_t)hipcomp::ParquetDeltaOutput::Offsets == pqd::kOffsets,
                  "ParquetDeltaOutput is the plan's Output");
    if (num_items > pqd::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (output != hipcomp::ParquetDeltaOutput::Values && output != hipcomp::ParquetDeltaOutput::Offsets)
      throw std::runtime_error(std::string(who) + ": unknown ParquetDeltaOutput");
    uint32_t element_bytes = 0;
    switch (out_type) {
    case HIPCOMP_TYPE_INT: element_bytes = 4; break;
    case HIPCOMP_TYPE_LONGLONG: element_bytes = 8; break;
    default: throw std::runtime_error(std::string(who) + ": the elements are INT or LONGLONG");
    }
    if (num_items == 0)
      return;
    if (!stream_ptrs || !stream_bytes || !out_ptrs || !out_caps || !statuses)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqd::Batch b;
    b.stream_ptrs = stream_ptrs;
    b.stream_bytes = stream_bytes;
    b.num_values = num_values;
    b.out_ptrs = out_ptrs;
    b.out_capacities = out_caps;
    b.value_counts = value_counts;
    b.consumed_bytes = consumed;
    b.statuses = statuses;
    b.items = num_items;
    b.output = (uint32_t)output;
    check(pqd::launch(b, element_bytes, stream), who);
  }

  // ---- a Parquet dictionary's entries gathered to rows (hipcomp/cascaded.hpp, index_parquet_dictionary,
  // gather_parquet_dictionary, gather_parquet_dictionary_strings; the arithmetic and the rules: parquet_dict_plan.hpp;
  // the kernels: parquet_dict_launch.hpp) ----
  // One launch each on the manager's stream: no scratch, no synchronisation, nothing of the host's read back.
  void dict_index_call(const uint8_t* const* dict_ptrs, const size_t* dict_bytes, const size_t* num_entries, int32_t* const* offset_ptrs,
                       const size_t* offset_caps, size_t* entry_counts, hipcompStatus_t* statuses, size_t num_dicts)
  {
    const char* const who = "index_parquet_dictionary";
    if (num_dicts > pqg::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (num_dicts == 0)
      return;
    if (!dict_ptrs || !dict_bytes || !num_entries || !offset_ptrs || !offset_caps || !statuses)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqg::IndexBatch b;
    b.dict_ptrs = dict_ptrs;
    b.dict_bytes = dict_bytes;
    b.num_entries = num_entries;
    b.offset_ptrs = offset_ptrs;
    b.offset_capacities = offset_caps;
    b.entry_counts = entry_counts;
    b.statuses = statuses;
    b.items = num_dicts;
    check(pqg::launch_index(b, stream), who);
  }
  // what the two gathers share: the checks of the rows' arrays, and those arrays into the batch
  static pqg::GatherBatch dict_rows(const char* who, const uint8_t* const* dict_ptrs, const size_t* dict_bytes, const size_t* dict_entries,
                                    const uint32_t* const* index_ptrs, const size_t* num_indices, const uint8_t* const* level_ptrs,
                                    const size_t* num_rows, const uint32_t* max_levels, uint8_t* const* validity_ptrs,
                                    hipcompStatus_t* statuses, size_t num_items)
  {
    if (!dict_ptrs || !dict_bytes || !dict_entries || !index_ptrs || !num_indices || !statuses)
      throw std::runtime_error(std::string(who) + ": a null array");
    if ((level_ptrs == nullptr) != (num_rows == nullptr) || (level_ptrs == nullptr) != (max_levels == nullptr))
      throw std::runtime_error(std::string(who) + ": the levels, the rows and the maximum levels come together");
    pqg::GatherBatch b = {};
    b.dict_ptrs = dict_ptrs;
    b.dict_bytes = dict_bytes;
    b.dict_entries = dict_entries;
    b.index_ptrs = index_ptrs;
    b.num_indices = num_indices;
    b.level_ptrs = level_ptrs;
    b.num_rows = num_rows;
    b.max_levels = max_levels;
    b.validity_ptrs = validity_ptrs;
    b.statuses = statuses;
    b.items = num_items;
    return b;
  }
  void dict_gather_call(const uint8_t* const* dict_ptrs, const size_t* dict_bytes, const size_t* dict_entries,
                        const uint32_t* const* index_ptrs, const size_t* num_indices, const uint8_t* const* level_ptrs,
                        const size_t* num_rows, const uint32_t* max_levels, void* const* out_ptrs, const size_t* out_caps,
                        uint8_t* const* validity_ptrs, hipcompStatus_t* statuses, size_t num_items, uint32_t entry_bytes)
  {
    const char* const who = "gather_parquet_dictionary";
    if (num_items > pqg::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (entry_bytes < 1 || entry_bytes > pqg::kMaxEntryBytes)
      throw std::runtime_error(std::string(who) + ": an entry has 1 to 64 bytes");
    if (num_items == 0)
      return;
    if (!out_ptrs || !out_caps)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqg::GatherBatch b = dict_rows(who, dict_ptrs, dict_bytes, dict_entries, index_ptrs, num_indices, level_ptrs, num_rows, max_levels,
                                   validity_ptrs, statuses, num_items);
    b.out_ptrs = out_ptrs;
    b.out_capacities = out_caps;
    b.entry_bytes = entry_bytes;
    check(pqg::launch_gather(b, stream), who);
  }
  void dict_strings_call(const uint8_t* const* dict_ptrs, const size_t* dict_bytes, const size_t* dict_entries,
                         const int32_t* const* dict_offsets, const uint32_t* const* index_ptrs, const size_t* num_indices,
                         const uint8_t* const* level_ptrs, const size_t* num_rows, const uint32_t* max_levels, int32_t* const* out_offsets,
                         const size_t* offset_caps, uint8_t* const* out_bytes, const size_t* byte_caps, size_t* out_byte_counts,
                         uint8_t* const* validity_ptrs, hipcompStatus_t* statuses, size_t num_items)
  {
    const char* const who = "gather_parquet_dictionary_strings";
    if (num_items > pqg::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (num_items == 0)
      return;
    if (!dict_offsets || !out_offsets || !offset_caps || !out_bytes || !byte_caps)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqg::GatherBatch b = dict_rows(who, dict_ptrs, dict_bytes, dict_entries, index_ptrs, num_indices, level_ptrs, num_rows, max_levels,
                                   validity_ptrs, statuses, num_items);
    b.dict_offsets = dict_offsets;
    b.out_offsets = out_offsets;
    b.offset_capacities = offset_caps;
    b.out_bytes = out_bytes;
    b.byte_capacities = byte_caps;
    b.out_byte_counts = out_byte_counts;
    check(pqg::launch_gather_strings(b, stream), who);
  }

  // ---- a Parquet page's dense values placed in rows (hipcomp/cascaded.hpp, place_parquet_values,
  // place_parquet_booleans, place_parquet_strings; the arithmetic and the rules: parquet_plain_plan.hpp; the kernels:
  // parquet_plain_launch.hpp) ----
  // One launch each on the manager's stream: no scratch, no synchronisation, nothing of the host's read back.
  // what the three share: the checks of the source's and the rows' arrays, and those arrays into the batch
  static pqv::PlaceBatch place_rows(const char* who, const uint8_t* const* src_ptrs, const size_t* src_bytes, const size_t* value_starts,
                                    const size_t* num_values, const uint8_t* const* level_ptrs, const size_t* num_rows,
                                    const uint32_t* max_levels, uint8_t* const* validity_ptrs, hipcompStatus_t* statuses, size_t num_items)
  {
    if (!src_ptrs || !src_bytes || !num_values || !statuses)
      throw std::runtime_error(std::string(who) + ": a null array");
    if ((level_ptrs == nullptr) != (num_rows == nullptr) || (level_ptrs == nullptr) != (max_levels == nullptr))
      throw std::runtime_error(std::string(who) + ": the levels, the rows and the maximum levels come together");
    pqv::PlaceBatch b = {};
    b.src_ptrs = src_ptrs;
    b.src_bytes = src_bytes;
    b.value_starts = value_starts;
    b.num_values = num_values;
    b.level_ptrs = level_ptrs;
    b.num_rows = num_rows;
    b.max_levels = max_levels;
    b.validity_ptrs = validity_ptrs;
    b.statuses = statuses;
    b.items = num_items;
    return b;
  }
  void place_values_call(const uint8_t* const* src_ptrs, const size_t* src_bytes, const size_t* value_starts, const size_t* num_values,
                         const uint8_t* const* level_ptrs, const size_t* num_rows, const uint32_t* max_levels, void* const* out_ptrs,
                         const size_t* out_caps, uint8_t* const* validity_ptrs, hipcompStatus_t* statuses, size_t num_items,
                         uint32_t value_bytes, hipcomp::ParquetValueLayout layout)
  {
    const char* const who = "place_parquet_values";
    static_assert((uint32_t)hipcomp::ParquetValueLayout::Plain == pqv::kPlain
                      && (uint32_t)hipcomp::ParquetValueLayout::ByteStreamSplit == pqv::kByteStreamSplit,
                  "ParquetValueLayout is the plan's ValueLayout");
    if (num_items > pqv::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (value_bytes < 1 || value_bytes > pqv::kMaxValueBytes)
      throw std::runtime_error(std::string(who) + ": a value has 1 to 64 bytes");
    if (layout != hipcomp::ParquetValueLayout::Plain && layout != hipcomp::ParquetValueLayout::ByteStreamSplit)
      throw std::runtime_error(std::string(who) + ": unknown ParquetValueLayout");
    if (num_items == 0)
      return;
    if (!out_ptrs || !out_caps)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqv::PlaceBatch b = place_rows(who, src_ptrs, src_bytes, value_starts, num_values, level_ptrs, num_rows, max_levels, validity_ptrs,
                                   statuses, num_items);
    b.out_ptrs = out_ptrs;
    b.out_capacities = out_caps;
    b.value_bytes = value_bytes;
    b.layout = (uint32_t)layout;
    check(pqv::launch_place_values(b, stream), who);
  }
  void place_booleans_call(const uint8_t* const* src_ptrs, const size_t* src_bytes, const size_t* value_starts, const size_t* num_values,
                           const uint8_t* const* level_ptrs, const size_t* num_rows, const uint32_t* max_levels, uint8_t* const* out_ptrs,
                           const size_t* out_caps, uint8_t* const* validity_ptrs, hipcompStatus_t* statuses, size_t num_items)
  {
    const char* const who = "place_parquet_booleans";
    if (num_items > pqv::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (num_items == 0)
      return;
    if (!out_ptrs || !out_caps)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqv::PlaceBatch b = place_rows(who, src_ptrs, src_bytes, value_starts, num_values, level_ptrs, num_rows, max_levels, validity_ptrs,
                                   statuses, num_items);
    b.out_ptrs = reinterpret_cast<void* const*>(out_ptrs);
    b.out_capacities = out_caps;
    check(pqv::launch_place_booleans(b, stream), who);
  }
  void place_strings_call(const uint8_t* const* body_ptrs, const size_t* body_bytes, const size_t* value_starts,
                          const int32_t* const* value_offsets, const size_t* num_values, const uint8_t* const* level_ptrs,
                          const size_t* num_rows, const uint32_t* max_levels, int32_t* const* out_offsets, const size_t* offset_caps,
                          uint8_t* const* out_bytes, const size_t* byte_caps, size_t* out_byte_counts, uint8_t* const* validity_ptrs,
                          hipcompStatus_t* statuses, size_t num_items, hipcomp::ParquetStringLayout layout)
  {
    const char* const who = "place_parquet_strings";
    static_assert((uint32_t)hipcomp::ParquetStringLayout::LengthPrefixed == pqv::kLengthPrefixed
                      && (uint32_t)hipcomp::ParquetStringLayout::Packed == pqv::kPacked,
                  "ParquetStringLayout is the plan's StringLayout");
    if (num_items > pqv::kMaxItems)
      throw std::runtime_error(std::string(who) + ": more than 2^20 items");
    if (layout != hipcomp::ParquetStringLayout::LengthPrefixed && layout != hipcomp::ParquetStringLayout::Packed)
      throw std::runtime_error(std::string(who) + ": unknown ParquetStringLayout");
    if (num_items == 0)
      return;
    if (!value_offsets || !out_offsets || !offset_caps || !out_bytes || !byte_caps)
      throw std::runtime_error(std::string(who) + ": a null array");
    pqv::PlaceBatch b = place_rows(who, body_ptrs, body_bytes, value_starts, num_values, level_ptrs, num_rows, max_levels, validity_ptrs,
                                   statuses, num_items);
    b.value_offsets = value_offsets;
    b.out_offsets = out_offsets;
    b.offset_capacities = offset_caps;
    b.out_bytes = out_bytes;
    b.byte_capacities = byte_caps;
    b.out_byte_counts = out_byte_counts;
    b.layout = (uint32_t)layout;
    check(pqv::launch_place_strings(b, stream), who);
  }

  // ---- a ranged read of seekable frames: bytes [first_byte, first_byte + num_bytes) of the content into out ----
  // The whole input has to be indexed frames: the hop and the test of every block in its place (no block is read for
  // it but its size word) say so on the device, and the host reads the frame table they leave -- the one
  // synchronisation of this call.  Then every frame the range touches is a ranged read of its own: range_plan.hpp
  // over the frame's content and block_bytes, the touched blocks listed from the index, decoded (the stored ones
  // copied), checked against their block checksums under a verifying policy, the two edge blocks through scratch
  // slots and range_kernels.hip's slices.
  void decompress_frame_range(uint8_t* out, const uint8_t* frames, size_t frames_bytes, const hipcomp::DecompressionConfig& cfg,
                              size_t first_byte, size_t num_bytes)
  {
    last_read_state = nullptr; // (until this call has a state of its own)
    // (a configuration refused by configure_frame_decompression: nothing to do, its status stands)
    if (cfg.num_chunks == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() != hipcompSuccess)
      return;
    if (first_byte > cfg.decomp_data_size || num_bytes > cfg.decomp_data_size - first_byte) {
      set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompErrorInvalidValue);
      check(hipGetLastError(), "decompress_frame_range kernels");
      return;
    }
    if (num_bytes == 0) {
      check(hipStreamSynchronize(stream), "decompress_frame_range");
      *cfg.get_status() = hipcompSuccess;
      return;
    }
    uint8_t* s = checksum_area(ensure_scratch(frame_read_bytes(1)));
    lz4f::ReadState* st = reinterpret_cast<lz4f::ReadState*>(s);
    lz4f::IndexState* ix = frame_index_state(s);
    last_read_state = st;
    std::unique_ptr<lz4f::IndexState> hx(new lz4f::IndexState);
    check(lz4f::launch_read_reset(st, stream), "decompress_frame_range");
    check(lz4f::launch_index_begin(frames, frames_bytes, ix, stream), "decompress_frame_range: index");
    check(lz4f::launch_index_list(frames, frames_bytes, ix, st, nullptr, 0, nullptr, 0, stream), "decompress_frame_range: index");
    check(hipMemcpyAsync(hx.get(), ix, sizeof(*hx), hipMemcpyDeviceToHost, stream), "decompress_frame_range");
    check(hipStreamSynchronize(stream), "decompress_frame_range");
    if (!hx->ok || hx->listed != hx->blocks) {
      *cfg.get_status() = hipcompErrorNotSupported;
      return;
    }
    if (hx->content_bytes != cfg.decomp_data_size || hx->blocks != cfg.num_chunks) { // (another input's configuration)
      *cfg.get_status() = hipcompErrorCannotDecompress;
      return;
    }
    // the frames the range touches, the largest block among them, the most blocks one of them contributes
    const uint64_t end = (uint64_t)first_byte + num_bytes;
    uint64_t stride = 16, most = 1;
    bool bare = false;
    for (uint32_t k = 0; k < hx->frames; ++k) {
      const lz4f::IndexedEntry& f = hx->frame[k];
      if (f.out_start >= end || f.out_start + f.content_bytes <= first_byte)
        continue;
      const uint64_t lo = (first_byte > f.out_start ? first_byte : f.out_start) - f.out_start;
      const uint64_t hi = (end < f.out_start + f.content_bytes ? end : f.out_start + f.content_bytes) - f.out_start;
      const uint64_t touched = (hi - 1) / f.block_bytes - lo / f.block_bytes + 1;
      most = touched > most ? touched : most;
      stride = ((uint64_t)f.block_bytes + 15) / 16 * 16 > stride ? ((uint64_t)f.block_bytes + 15) / 16 * 16 : stride;
      bare = bare || !(f.flags & lz4f::kBlockSum);
    }
    // scratch: the fixed part, two slots, the entry lists of a pass
    const size_t fixed = kFrameReadFixed + 2 * (size_t)stride + 16;
    const size_t room = scratch_bytes();
    // (frames of blocks so much larger than this manager's chunks that its scratch space does not hold two of them:
    // a limit of this manager, reported like the other one, kMaxIndexedFrames; the stream is idle, nothing is written)
    if (room < fixed + lz4f::kReadEntryBytes) {
      *cfg.get_status() = hipcompErrorNotSupported;
      return;
    }
    size_t P = (room - fixed) / lz4f::kReadEntryBytes;
    P = P < kPlacedSlab ? P : kPlacedSlab;
    P = most < P ? (size_t)most : P;
    s = checksum_area(ensure_scratch(fixed + lz4f::kReadEntryBytes * P));
    st = reinterpret_cast<lz4f::ReadState*>(s);
    last_read_state = st;
    ix = frame_index_state(s);
    // (the scratch may have moved: the state the kernels read is written again)
    check(hipMemcpyAsync(ix, hx.get(), sizeof(*hx), hipMemcpyHostToDevice, stream), "decompress_frame_range");
    check(lz4f::launch_read_reset(st, stream), "decompress_frame_range");
    void* const ticket = s + 128;
    RangeSlots slots;
    slots.base = checksum_area(s + kFrameReadLists);
    slots.stride = stride;
    const lz4f::ReadLists l = frame_read_lists(slots.base + 2 * stride, P);
    for (uint32_t k = 0; k < hx->frames; ++k) {
      const lz4f::IndexedEntry& f = hx->frame[k];
      if (f.out_start >= end || f.out_start + f.content_bytes <= first_byte)
        continue;
      const uint64_t lo = (first_byte > f.out_start ? first_byte : f.out_start) - f.out_start;
      const uint64_t hi = (end < f.out_start + f.content_bytes ? end : f.out_start + f.content_bytes) - f.out_start;
      uint8_t* const out_f = out + (f.out_start + lo - first_byte);
      range::Plan plan;
      if (!range::range_plan(plan, f.content_bytes, f.block_bytes, lo, hi - lo, (uint32_t)P, 2, 1, 0, 1))
        throw std::runtime_error("decompress_frame_range: no plan"); // (lo < hi <= content_bytes: not reached)
      for (uint64_t pass = 0; pass < plan.passes; ++pass) {
        const uint64_t first = range::range_pass_first(plan, pass);
        const uint32_t count = range::range_pass_count(plan, pass);
        check(lz4f::launch_index_range_list(frames, frames_bytes, ix, k, plan, first, count, out_f, slots, l, st, stream),
              "decompress_frame_range: block list");
        check(lz4_launch_decompress(l.comp_ptrs, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, true,
                                    stream, ticket, 64),
              "LZ4Manager::decompress_frame_range");
        check(lz4f::launch_read_verdict(l, st, count, stream), "decompress_frame_range: verdict");
        check(lz4f::launch_read_stored(l, st, count, 2 * (uint64_t)f.block_bytes, stream), "decompress_frame_range: stored blocks");
        check(lz4f::launch_index_range_settle(l, st, count, stream), "decompress_frame_range: stored blocks");
        if (verifies())
          check(lz4f::launch_read_block_sums(l, st, count, stream), "decompress_frame_range: block checksums");
        // (the edge blocks are in a frame's first and last pass)
        if (pass == 0 || pass + 1 == plan.passes)
          check(range_launch_slices(plan, first, count, out_f, slots, l.statuses, l.actual, l.caps, stream),
                "decompress_frame_range: slices");
      }
    }
    check(lz4f::launch_index_range_finish(st, policy == hipcomp::ComputeAndVerify && bare, cfg.get_status(), stream),
          "decompress_frame_range");
    check(hipGetLastError(), "decompress_frame_range kernels");
  }

  // ---- Snappy framed streams (hipcomp/snappy.hpp; the format: snappy_frame.hpp; the kernels: snappy_frame_launch.hpp;
  // DESIGN.md 21) ----
  // Passes of as many chunks as fit the scratch space scratch_bytes() promises, like the LZ4 frames above.
  // Writing, a pass of P chunks: the stream cursor (16 bytes), six lists, a slot per chunk for the batched encoder
  // (unplaced: the stream wants the chunks in order and the stored ones from the input).
  size_t sz_write_bytes(size_t P) const { return 16 + 16 + szf::kWriteEntryBytes * P + 16 + P * slot_bytes; }
  size_t sz_write_pass(size_t chunks) const
  {
    const size_t room = scratch_bytes();
    size_t P = chunks < kPlacedSlab ? (chunks ? chunks : 1) : kPlacedSlab;
    if (sz_write_bytes(P) <= room)
      return P;
    size_t lo = 1; // (fits: scratch_bytes() holds a slot per resident wave and a full pass's lists)
    while (lo < P) {
      const size_t mid = lo + (P - lo + 1) / 2;
      if (sz_write_bytes(mid) <= room)
        lo = mid;
      else
        P = mid - 1;
    }
    return lo;
  }
  // Reading, a pass of P chunks: the walk's state (128 bytes), the indexed read's state
  // (snappy_frame_index_launch.hpp), the entry lists.  The required scratch is what it was, so a pass of every
  // framed read, indexed or not, holds 1664 / kReadEntryBytes = 30 entries fewer than before the index.
  static constexpr size_t kSzReadLists = 1792;
  static constexpr size_t kSzReadFixed = 16 + kSzReadLists;
  static_assert(128 + sizeof(szf::IndexState) <= kSzReadLists, "the indexed read's state does not fit");
  static szf::IndexState* sz_index_state(uint8_t* s) { return reinterpret_cast<szf::IndexState*>(s + 128); }
  size_t sz_read_bytes(size_t P) const { return kSzReadFixed + szf::kReadEntryBytes * P; }
  size_t sz_read_pass(size_t chunks) const
  {
    size_t P = (scratch_bytes() - kSzReadFixed) / szf::kReadEntryBytes;
    P = P < kPlacedSlab ? P : kPlacedSlab;
    return chunks < P ? (chunks ? chunks : 1) : P;
  }
  static szf::ReadLists sz_read_lists(uint8_t* at, size_t P)
  {
    szf::ReadLists l;
    l.payloads = reinterpret_cast<const uint8_t**>(at);
    l.batch_bytes = reinterpret_cast<size_t*>(at + 8 * P);
    l.out_ptrs = reinterpret_cast<uint8_t**>(at + 16 * P);
    l.batch_caps = reinterpret_cast<size_t*>(at + 24 * P);
    l.actual = reinterpret_cast<size_t*>(at + 32 * P);
    l.content = reinterpret_cast<uint32_t*>(at + 40 * P);
    l.crcs = reinterpret_cast<uint32_t*>(at + 44 * P);
    l.flags = reinterpret_cast<uint32_t*>(at + 48 * P);
    l.statuses = reinterpret_cast<hipcompStatus_t*>(at + 52 * P);
    return l;
  }

  // index: the stream gets its chunk index behind the identifier (snappy_frame_index.hpp), 40 + 4 * num_chunks
  // bytes more
  hipcomp::CompressionConfig sz_configure_compression(size_t decomp_buffer_size, bool index = false) const
  {
    hipcomp::CompressionConfig c(decomp_buffer_size);
    // no data chunk of the format holds a chunk; the index's length field does not hold the words
    if (chunk_bytes > szf::kMaxContent
        || (index && (decomp_buffer_size + chunk_bytes - 1) / chunk_bytes > szf::kIndexMaxChunks)) {
      *c.get_status() = hipcompErrorInvalidValue;
      return c;
    }
    c.num_chunks = (decomp_buffer_size + chunk_bytes - 1) / chunk_bytes;
    c.max_compressed_buffer_size =
        (size_t)(index ? szf::indexed_frame_bound(c.num_chunks, chunk_bytes) : szf::frame_bound(c.num_chunks, chunk_bytes));
    return c;
  }

  // index: the room of the index is left behind the identifier, its words are written pass by pass from the lists
  // the chunks are written from, its CRC when they all stand
  void sz_compress(const uint8_t* decomp_buffer, uint8_t* frame, const hipcomp::CompressionConfig& cfg, size_t* frame_bytes,
                   bool index = false)
  {
    if (reinterpret_cast<uintptr_t>(frame_bytes) & 7)
      throw std::runtime_error("compress_frame: frame_bytes must be 8-byte aligned");
    if (chunk_bytes > szf::kMaxContent
        || (index && (cfg.uncompressed_buffer_size + chunk_bytes - 1) / chunk_bytes > szf::kIndexMaxChunks)) {
      set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompErrorInvalidValue);
      check(szf::launch_set_size(frame_bytes, 0, stream), "compress_frame");
      return;
    }
    const size_t n = cfg.num_chunks;
    const size_t P = sz_write_pass(n);
    uint8_t* const s = checksum_area(ensure_scratch(sz_write_bytes(P)));
    unsigned long long* const cursor = reinterpret_cast<unsigned long long*>(s);
    uint8_t* const lists = s + 16;
    szf::WriteLists l;
    l.in_ptrs = reinterpret_cast<const uint8_t**>(lists);
    l.in_bytes = reinterpret_cast<size_t*>(lists + 8 * P);
    l.slots = reinterpret_cast<uint8_t**>(lists + 16 * P);
    l.block_bytes = reinterpret_cast<size_t*>(lists + 24 * P);
    l.offsets = reinterpret_cast<uint64_t*>(lists + 32 * P);
    l.crcs = reinterpret_cast<uint32_t*>(lists + 40 * P);
    uint8_t* const slots = checksum_area(lists + szf::kWriteEntryBytes * P);
    set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompSuccess);
    uint8_t* const index_at = frame + szf::kIdentifierBytes;
    if (index)
      check(szf::launch_index_write_begin(frame, cursor, (uint32_t)n, (uint32_t)chunk_bytes, cfg.uncompressed_buffer_size, stream),
            "compress_frame: index");
    else
      check(szf::launch_write_begin(frame, cursor, stream), "compress_frame: identifier");
    for (size_t first = 0; first < n; first += P) {
      const uint32_t count = (uint32_t)(n - first < P ? n - first : P);
      check(szf::launch_write_lists(decomp_buffer, cfg.uncompressed_buffer_size, chunk_bytes, first, count, slots, slot_bytes,
                                    l, stream),
            "compress_frame: chunk lists");
      snappy_launch_compress(l.in_ptrs, l.in_bytes, l.slots, l.block_bytes, count, stream);
      check(hipGetLastError(), "SnappyManager::compress_frame");
      // (the CRC is part of the format: computed under every ChecksumPolicy)
      check(szf::launch_write_crcs(l, count, stream), "compress_frame: checksums");
      check(szf::launch_write_scan(l, count, cursor, stream), "compress_frame: scan");
      check(szf::launch_write_chunks(frame, l, count, chunk_bytes, stream), "compress_frame: chunks");
      if (index)
        check(szf::launch_index_write_words(index_at, l, first, count, stream), "compress_frame: index");
    }
    if (index)
      check(szf::launch_index_write_end(index_at, (uint32_t)n, stream), "compress_frame: index");
    check(szf::launch_write_end(cursor, frame_bytes, stream), "compress_frame: length");
    check(hipGetLastError(), "compress_frame kernels");
  }

  // What configure_frame_decompression found in the buffer it saw last: decompress_frame does not launch the
  // indexed passes for a buffer that had no index then.  A hint and no more -- the passes themselves decide on the
  // device, whatever the buffer holds by now.
  const uint8_t* sz_hint_frames = nullptr;
  size_t sz_hint_bytes = 0;
  bool sz_hint_indexed = false;
  // the state of the last decompress_frame or decompress_frame_range
  szf::ReadState* sz_last_read_state = nullptr;

  // Data chunks the chain's walk stepped over in the last decompress_frame or decompress_frame_range (synchronises
  // the stream): ReadState::walked, which the walk alone adds to.
  size_t sz_walked_chunks()
  {
    if (!sz_last_read_state)
      return 0;
    szf::ReadState h;
    check(hipMemcpyAsync(&h, sz_last_read_state, sizeof(h), hipMemcpyDeviceToHost, stream), "get_frame_walked_chunks");
    check(hipStreamSynchronize(stream), "get_frame_walked_chunks");
    return (size_t)h.walked;
  }

  hipcomp::DecompressionConfig sz_configure_decompression(const uint8_t* frames, size_t frames_bytes)
  {
    hipcomp::DecompressionConfig d;
    uint8_t* const s = checksum_area(ensure_scratch(sz_read_bytes(1)));
    szf::ReadState* const st = reinterpret_cast<szf::ReadState*>(s);
    szf::ReadState h;
    // indexed units and nothing else: the numbers are the indexes', every chunk tested in its place
    {
      szf::IndexState* const ix = sz_index_state(s);
      szf::IndexState hx;
      check(szf::launch_index_begin(frames, frames_bytes, ix, stream), "configure_frame_decompression: index");
      check(szf::launch_index_list(frames, frames_bytes, ix, st, nullptr, 0, stream), "configure_frame_decompression: index");
      check(hipMemcpyAsync(&hx, ix, offsetof(szf::IndexState, unit), hipMemcpyDeviceToHost, stream),
            "configure_frame_decompression");
      check(hipStreamSynchronize(stream), "configure_frame_decompression");
      sz_hint_frames = frames;
      sz_hint_bytes = frames_bytes;
      sz_hint_indexed = hx.ok && hx.listed == hx.chunks;
      if (sz_hint_indexed) {
        d.num_chunks = (uint32_t)hx.chunks;
        d.decomp_data_size = (size_t)hx.content_bytes;
        return d;
      }
    }
    check(szf::launch_read_reset(st, stream), "configure_frame_decompression");
    check(szf::launch_read_walk(frames, frames_bytes, st, nullptr, 0, stream), "configure_frame_decompression");
    check(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, stream), "configure_frame_decompression");
    check(hipStreamSynchronize(stream), "configure_frame_decompression");
    if (h.reason != szf::kOk || h.chunks > 0xFFFFFFFFull) {
      *d.get_status() = hipcompErrorCannotDecompress;
      return d;
    }
    d.num_chunks = (uint32_t)h.chunks;
    d.decomp_data_size = (size_t)h.content;
    return d;
  }

  void sz_decompress(uint8_t* decomp_buffer, const uint8_t* frames, size_t frames_bytes, const hipcomp::DecompressionConfig& cfg)
  {
    // (a configuration refused by configure_frame_decompression: nothing to do, its status stands)
    if (cfg.num_chunks == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() != hipcompSuccess)
      return;
    const size_t chunks = cfg.num_chunks, P = sz_read_pass(chunks);
    uint8_t* const s = checksum_area(ensure_scratch(sz_read_bytes(P)));
    szf::ReadState* const st = reinterpret_cast<szf::ReadState*>(s);
    // (no indexed passes for a buffer that had no index when it was configured: the launches of a manager without
    // the index, one for one)
    const bool try_index = !(sz_hint_frames == frames && sz_hint_bytes == frames_bytes && !sz_hint_indexed);
    szf::IndexState* const ix = try_index ? sz_index_state(s) : nullptr;
    sz_last_read_state = st;
    const szf::ReadLists l = sz_read_lists(s + kSzReadLists, P);
    check(szf::launch_read_reset(st, stream), "decompress_frame");
    // The indexed passes: entries from the index (no walk), the placing scan, the batched decoder, the stored chunks,
    // the CRCs.  Whether they held is a word on the device: if so the chain's passes below find nothing to do, if
    // not they start from the reset state and do it all.
    if (try_index) {
      check(szf::launch_index_begin(frames, frames_bytes, ix, stream), "decompress_frame: index");
      for (size_t first = 0; first < chunks; first += P) {
        const uint32_t count = (uint32_t)(chunks - first < P ? chunks - first : P);
        check(szf::launch_index_list(frames, frames_bytes, ix, st, &l, count, stream), "decompress_frame: index");
        check(szf::launch_read_scan(l, st, decomp_buffer, cfg.decomp_data_size, stream), "decompress_frame: scan");
        snappy_launch_decompress(l.payloads, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, stream);
        check(hipGetLastError(), "SnappyManager::decompress_frame");
        check(szf::launch_index_verdict(l, st, ix, count, stream), "decompress_frame: index");
        check(szf::launch_read_stored(l, st, count, 2 * (uint64_t)(cfg.decomp_data_size / chunks), stream),
              "decompress_frame: stored chunks");
        if (verifies())
          check(szf::launch_read_crcs(l, st, count, stream), "decompress_frame: checksums");
      }
      check(szf::launch_index_end(ix, st, l, (uint32_t)(chunks < P ? chunks : P), frames, frames_bytes, chunks, stream),
            "decompress_frame: index");
    }
    const uint32_t* const skip = ix ? &ix->skip : nullptr;
    if (chunks == 0) // identifiers and padding at the most
      check(szf::launch_read_walk(frames, frames_bytes, st, &l, 0, stream, skip), "decompress_frame: walk");
    for (size_t first = 0; first < chunks; first += P) {
      const uint32_t count = (uint32_t)(chunks - first < P ? chunks - first : P);
      check(szf::launch_read_walk(frames, frames_bytes, st, &l, count, stream, skip), "decompress_frame: walk");
      check(szf::launch_read_scan(l, st, decomp_buffer, cfg.decomp_data_size, stream), "decompress_frame: scan");
      snappy_launch_decompress(l.payloads, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, stream);
      check(hipGetLastError(), "SnappyManager::decompress_frame");
      check(szf::launch_read_verdict(l, st, count, stream), "decompress_frame: verdict");
      // (workgroups per stored chunk by the size of the average chunk: the sizes themselves are on the device)
      check(szf::launch_read_stored(l, st, count, 2 * (uint64_t)(cfg.decomp_data_size / chunks), stream),
            "decompress_frame: stored chunks");
      if (verifies())
        check(szf::launch_read_crcs(l, st, count, stream), "decompress_frame: checksums");
    }
    check(szf::launch_read_finish(st, chunks, cfg.decomp_data_size, cfg.get_status(), stream), "decompress_frame");
    check(hipGetLastError(), "decompress_frame kernels");
  }

  // ---- a ranged read of seekable streams: bytes [first_byte, first_byte + num_bytes) of the content into out ----
  // The whole input has to be indexed units: the hop and the test of every chunk in its place (of no chunk more is
  // read for it than its first 16 bytes) say so on the device, and the host reads the unit table they leave -- the
  // one synchronisation of this call.  Then every unit the range touches is a ranged read of its own: range_plan.hpp
  // over the unit's content and chunk_bytes, the touched chunks listed from the index, decoded (the stored ones
  // copied), checked against their CRCs under a verifying policy, the two edge chunks through scratch slots and
  // range_kernels.hip's slices.
  void sz_decompress_range(uint8_t* out, const uint8_t* frames, size_t frames_bytes, const hipcomp::DecompressionConfig& cfg,
                           size_t first_byte, size_t num_bytes)
  {
    sz_last_read_state = nullptr; // (until this call has a state of its own)
    // (a configuration refused by configure_frame_decompression: nothing to do, its status stands)
    if (cfg.num_chunks == 0 && cfg.decomp_data_size == 0 && *cfg.get_status() != hipcompSuccess)
      return;
    if (first_byte > cfg.decomp_data_size || num_bytes > cfg.decomp_data_size - first_byte) {
      set_status_kernel<<<1, 1, 0, stream>>>(cfg.get_status(), hipcompErrorInvalidValue);
      check(hipGetLastError(), "decompress_frame_range kernels");
      return;
    }
    if (num_bytes == 0) {
      check(hipStreamSynchronize(stream), "decompress_frame_range");
      *cfg.get_status() = hipcompSuccess;
      return;
    }
    uint8_t* s = checksum_area(ensure_scratch(sz_read_bytes(1)));
    szf::ReadState* st = reinterpret_cast<szf::ReadState*>(s);
    szf::IndexState* ix = sz_index_state(s);
    sz_last_read_state = st;
    std::unique_ptr<szf::IndexState> hx(new szf::IndexState);
    check(szf::launch_read_reset(st, stream), "decompress_frame_range");
    check(szf::launch_index_begin(frames, frames_bytes, ix, stream), "decompress_frame_range: index");
    check(szf::launch_index_list(frames, frames_bytes, ix, st, nullptr, 0, stream), "decompress_frame_range: index");
    check(hipMemcpyAsync(hx.get(), ix, sizeof(*hx), hipMemcpyDeviceToHost, stream), "decompress_frame_range");
    check(hipStreamSynchronize(stream), "decompress_frame_range");
    if (!hx->ok || hx->listed != hx->chunks) {
      *cfg.get_status() = hipcompErrorNotSupported;
      return;
    }
    if (hx->content_bytes != cfg.decomp_data_size || hx->chunks != cfg.num_chunks) { // (another input's configuration)
      *cfg.get_status() = hipcompErrorCannotDecompress;
      return;
    }
    // the units the range touches, the largest chunk among them, the most chunks one of them contributes
    const uint64_t end = (uint64_t)first_byte + num_bytes;
    uint64_t stride = 16, most = 1;
    for (uint32_t k = 0; k < hx->units; ++k) {
      const szf::IndexedEntry& f = hx->unit[k];
      if (f.out_start >= end || f.out_start + f.content_bytes <= first_byte)
        continue;
      const uint64_t lo = (first_byte > f.out_start ? first_byte : f.out_start) - f.out_start;
      const uint64_t hi = (end < f.out_start + f.content_bytes ? end : f.out_start + f.content_bytes) - f.out_start;
      const uint64_t touched = (hi - 1) / f.chunk_bytes - lo / f.chunk_bytes + 1;
      most = touched > most ? touched : most;
      stride = ((uint64_t)f.chunk_bytes + 15) / 16 * 16 > stride ? ((uint64_t)f.chunk_bytes + 15) / 16 * 16 : stride;
    }
    // scratch: the fixed part, two slots, the entry lists of a pass with a size_t more per entry (the shares, for
    // the slices)
    const size_t fixed = kSzReadFixed + 2 * (size_t)stride + 16, entry = szf::kReadEntryBytes + 8;
    const size_t room = scratch_bytes();
    // (units of chunks so much larger than this manager's that its scratch space does not hold two of them: a limit
    // of this manager, reported like the other one, kMaxIndexedStreams; the stream is idle, nothing is written)
    if (room < fixed + entry) {
      *cfg.get_status() = hipcompErrorNotSupported;
      return;
    }
    size_t P = (room - fixed) / entry;
    P = P < kPlacedSlab ? P : kPlacedSlab;
    P = most < P ? (size_t)most : P;
    s = checksum_area(ensure_scratch(fixed + entry * P));
    st = reinterpret_cast<szf::ReadState*>(s);
    sz_last_read_state = st;
    ix = sz_index_state(s);
    // (the scratch may have moved: the state the kernels read is written again)
    check(hipMemcpyAsync(ix, hx.get(), sizeof(*hx), hipMemcpyHostToDevice, stream), "decompress_frame_range");
    check(szf::launch_read_reset(st, stream), "decompress_frame_range");
    RangeSlots slots;
    slots.base = checksum_area(s + kSzReadLists);
    slots.stride = stride;
    size_t* const caps = reinterpret_cast<size_t*>(slots.base + 2 * stride);
    const szf::ReadLists l = sz_read_lists(slots.base + 2 * stride + 8 * P, P);
    for (uint32_t k = 0; k < hx->units; ++k) {
      const szf::IndexedEntry& f = hx->unit[k];
      if (f.out_start >= end || f.out_start + f.content_bytes <= first_byte)
        continue;
      const uint64_t lo = (first_byte > f.out_start ? first_byte : f.out_start) - f.out_start;
      const uint64_t hi = (end < f.out_start + f.content_bytes ? end : f.out_start + f.content_bytes) - f.out_start;
      uint8_t* const out_f = out + (f.out_start + lo - first_byte);
      range::Plan plan;
      if (!range::range_plan(plan, f.content_bytes, f.chunk_bytes, lo, hi - lo, (uint32_t)P, 2, 1, 0, 1))
        throw std::runtime_error("decompress_frame_range: no plan"); // (lo < hi <= content_bytes: not reached)
      for (uint64_t pass = 0; pass < plan.passes; ++pass) {
        const uint64_t first = range::range_pass_first(plan, pass);
        const uint32_t count = range::range_pass_count(plan, pass);
        check(szf::launch_index_range_list(frames, frames_bytes, ix, k, plan, first, count, out_f, slots, l, caps, st, stream),
              "decompress_frame_range: chunk list");
        snappy_launch_decompress(l.payloads, l.batch_bytes, l.batch_caps, count, l.out_ptrs, l.actual, l.statuses, stream);
        check(hipGetLastError(), "SnappyManager::decompress_frame_range");
        check(szf::launch_read_verdict(l, st, count, stream), "decompress_frame_range: verdict");
        check(szf::launch_read_stored(l, st, count, 2 * (uint64_t)f.chunk_bytes, stream), "decompress_frame_range: stored chunks");
        check(szf::launch_index_range_settle(l, caps, st, count, stream), "decompress_frame_range: stored chunks");
        if (verifies())
          check(szf::launch_read_crcs(l, st, count, stream), "decompress_frame_range: checksums");
        // (the edge chunks are in a unit's first and last pass)
        if (pass == 0 || pass + 1 == plan.passes)
          check(range_launch_slices(plan, first, count, out_f, slots, l.statuses, l.actual, caps, stream),
                "decompress_frame_range: slices");
      }
    }
    check(szf::launch_index_range_finish(st, cfg.get_status(), stream), "decompress_frame_range");
    check(hipGetLastError(), "decompress_frame_range kernels");
  }

  void set_scratch_buffer(uint8_t* new_scratch_buffer)
  {
    if (own_scratch)
      (void)hipFree(scratch);
    own_scratch = false;
    own_capacity = 0;
    scratch = new_scratch_buffer;
  }

  size_t compressed_output_size(const uint8_t* comp_buffer)
  {
    const CommonHeader& h = read_header(comp_buffer);
    return (size_t)(h.comp_data_size + h.comp_data_offset);
  }
};

hipcomp::DecompressionConfig config_of(const hipcomp::CompressionConfig& comp_config)
{
  hipcomp::DecompressionConfig d;
  d.decomp_data_size = comp_config.uncompressed_buffer_size;
  d.num_chunks = (uint32_t)comp_config.num_chunks;
  return d;
}

} // namespace hlif
} // namespace hcamd

namespace hipcomp
{
using namespace hcamd;
using namespace hcamd::hlif;

CompressionConfig::CompressionConfig(size_t n)
    : uncompressed_buffer_size(n), max_compressed_buffer_size(0), num_chunks(0), status(new_status())
{
}
hipcompStatus_t* CompressionConfig::get_status() const { return status.get(); }
DecompressionConfig::DecompressionConfig() : decomp_data_size(0), num_chunks(0), status(new_status()) {}
hipcompStatus_t* DecompressionConfig::get_status() const { return status.get(); }

// the eight virtuals of a manager, all on its core
#define HCAMD_MANAGER_METHODS(M)                                                                                    \
  M::~M() {}                                                                                                        \
  CompressionConfig M::configure_compression(const size_t n) { return impl->core.configure_compression(n); }       \
  void M::compress(const uint8_t* in, uint8_t* out, const CompressionConfig& c) { impl->core.compress(in, out, c); } \
  DecompressionConfig M::configure_decompression(const uint8_t* comp) { return impl->core.configure_decompression(comp); } \
  DecompressionConfig M::configure_decompression(const CompressionConfig& c) { return config_of(c); }              \
  void M::decompress(uint8_t* out, const uint8_t* comp, const DecompressionConfig& c) { impl->core.decompress(out, comp, c); } \
  void M::set_scratch_buffer(uint8_t* p) { impl->core.set_scratch_buffer(p); }                                      \
  size_t M::get_required_scratch_buffer_size() { return impl->core.scratch_bytes(); }                               \
  size_t M::get_compressed_output_size(uint8_t* comp) { return impl->core.compressed_output_size(comp); }                         \
  void M::decompress_range(uint8_t* out, const uint8_t* comp, const DecompressionConfig& c, size_t first_byte,      \
                           size_t num_bytes)                                                                        \
  {                                                                                                                 \
    impl->core.decompress_range(out, comp, c, first_byte, num_bytes);                                               \
  }                                                                                                                 \
  void M::decompress_ranges(uint8_t* out, size_t out_bytes, const uint8_t* comp, const DecompressionConfig& c,      \
                            const size_t* device_first_bytes, const size_t* device_num_bytes, size_t num_ranges,    \
                            size_t* device_out_offsets)                                                             \
  {                                                                                                                 \
    impl->core.decompress_ranges(out, out_bytes, comp, c, device_first_bytes, device_num_bytes, num_ranges,         \
                                 device_out_offsets);                                                               \
  }                                                                                                                 \
  size_t M::get_ranges_pass_chunks() const { return impl->core.ranges_pass_chunks(); }                              \
  RangesStats M::get_ranges_stats() const { return impl->core.ranges_stats; }

struct LZ4Manager::Impl
{
  Core core;
  Impl(size_t chunk, hipStream_t st, int dev) : core(Core::LZ4, chunk, st, dev, "LZ4Manager") {}
};
struct SnappyManager::Impl
{
  Core core;
  Impl(size_t chunk, hipStream_t st, int dev) : core(Core::Snappy, chunk, st, dev, "SnappyManager") {}
};
struct CascadedManager::Impl
{
  Core core;
  Impl(size_t chunk, hipStream_t st, int dev) : core(Core::Cascaded, chunk, st, dev, "CascadedManager") {}
};

LZ4Manager::LZ4Manager(size_t uncomp_chunk_size, hipcompType_t data_type, hipStream_t user_stream, const int device_id)
{
  if (uncomp_chunk_size == 0 || uncomp_chunk_size > (size_t(1) << 24))
    throw std::runtime_error("LZ4Manager: uncomp_chunk_size must be in [1, 16 MiB]");
  size_t slot = 0;
  if (hipcompBatchedLZ4CompressGetMaxOutputChunkSize(uncomp_chunk_size, hipcompBatchedLZ4Opts_t{data_type}, &slot)
      != hipcompSuccess)
    throw std::runtime_error("LZ4Manager: bad chunk size");
  int elem = 0;
  switch (data_type) {
  case HIPCOMP_TYPE_BITS: case HIPCOMP_TYPE_CHAR: case HIPCOMP_TYPE_UCHAR: elem = 1; break;
  case HIPCOMP_TYPE_SHORT: case HIPCOMP_TYPE_USHORT: elem = 2; break;
  case HIPCOMP_TYPE_INT: case HIPCOMP_TYPE_UINT: elem = 4; break;
  default: throw std::runtime_error("LZ4Manager: unsupported data type");
  }
  impl.reset(new Impl(uncomp_chunk_size, user_stream, device_id));
  Core& m = impl->core;
  m.format = kLZ4;
  m.format_header_bytes = sizeof(LZ4FormatSpecHeader);
  const uint32_t t = (uint32_t)data_type;
  std::memcpy(m.format_header.bytes, &t, sizeof(t));
  m.lz4_type = data_type;
  m.lz4_elem = elem;
  size_t p = 1;
  while (p < uncomp_chunk_size)
    p *= 2;
  m.ht_size = (uint32_t)(p < 16384 ? p : 16384);
  m.finish_init(slot);
}
LZ4Manager::LZ4Manager(size_t uncomp_chunk_size, hipcompType_t data_type, hipStream_t user_stream, const int device_id,
                       ChecksumPolicy checksum_policy)
    : LZ4Manager(uncomp_chunk_size, data_type, user_stream, device_id)
{
  impl->core.set_policy(checksum_policy);
}
HCAMD_MANAGER_METHODS(LZ4Manager)
CompressionConfig LZ4Manager::configure_frame_compression(size_t n) { return impl->core.configure_frame_compression(n); }
CompressionConfig LZ4Manager::configure_frame_compression(size_t n, LZ4FrameIndex index)
{
  return impl->core.configure_frame_compression(n, index == LZ4FrameIndex::Leading);
}
void LZ4Manager::compress_frame(const uint8_t* in, uint8_t* frame, const CompressionConfig& c, size_t* frame_bytes,
                                LZ4FrameIndex index)
{
  impl->core.compress_frame(in, frame, c, frame_bytes, index == LZ4FrameIndex::Leading);
}
size_t LZ4Manager::get_frame_walked_blocks() { return impl->core.frame_walked_blocks(); }
void LZ4Manager::decompress_frame_range(uint8_t* out, const uint8_t* frames, size_t frames_bytes, const DecompressionConfig& c,
                                        size_t first_byte, size_t num_bytes)
{
  impl->core.decompress_frame_range(out, frames, frames_bytes, c, first_byte, num_bytes);
}
void LZ4Manager::decompress_frames(const uint8_t* const* device_item_ptrs, const size_t* device_item_bytes,
                                   uint8_t* const* device_out_ptrs, const size_t* device_out_capacities,
                                   size_t* device_actual_bytes, hipcompStatus_t* device_statuses, size_t num_items,
                                   LZ4FramePrefix prefix)
{
  impl->core.frames_call(device_item_ptrs, device_item_bytes, device_out_ptrs, device_out_capacities, device_actual_bytes,
                         device_statuses, num_items, prefix == LZ4FramePrefix::ArrowLength ? lz4fb::kArrowLength : lz4fb::kNone,
                         true, "decompress_frames");
}
void LZ4Manager::get_frames_decompressed_sizes(const uint8_t* const* device_item_ptrs, const size_t* device_item_bytes,
                                               size_t* device_decompressed_bytes, size_t num_items, LZ4FramePrefix prefix)
{
  impl->core.frames_call(device_item_ptrs, device_item_bytes, nullptr, nullptr, device_decompressed_bytes, nullptr, num_items,
                         prefix == LZ4FramePrefix::ArrowLength ? lz4fb::kArrowLength : lz4fb::kNone, false,
                         "get_frames_decompressed_sizes");
}
void LZ4Manager::set_frames_pass_entries(size_t entries) { impl->core.frames_pass_limit = entries; }
LZ4FramesStats LZ4Manager::get_frames_stats() const { return impl->core.frames_stats; }
void LZ4Manager::compress_frame(const uint8_t* in, uint8_t* frame, const CompressionConfig& c, size_t* frame_bytes)
{
  impl->core.compress_frame(in, frame, c, frame_bytes);
}
DecompressionConfig LZ4Manager::configure_frame_decompression(const uint8_t* frames, size_t frames_bytes)
{
  return impl->core.configure_frame_decompression(frames, frames_bytes);
}
void LZ4Manager::decompress_frame(uint8_t* out, const uint8_t* frames, size_t frames_bytes, const DecompressionConfig& c)
{
  impl->core.decompress_frame(out, frames, frames_bytes, c);
}

SnappyManager::SnappyManager(size_t uncomp_chunk_size, hipStream_t user_stream, int device_id)
{
  size_t slot = 0;
  if (uncomp_chunk_size == 0
      || hipcompBatchedSnappyCompressGetMaxOutputChunkSize(uncomp_chunk_size, hipcompBatchedSnappyDefaultOpts, &slot)
             != hipcompSuccess)
    throw std::runtime_error("SnappyManager: bad chunk size");
  impl.reset(new Impl(uncomp_chunk_size, user_stream, device_id));
  Core& m = impl->core;
  m.format = kSnappy;
  m.format_header_bytes = sizeof(SnappyFormatSpecHeader); // 1: an empty struct
  m.finish_init(slot);
}
SnappyManager::SnappyManager(size_t uncomp_chunk_size, hipStream_t user_stream, int device_id, ChecksumPolicy checksum_policy)
    : SnappyManager(uncomp_chunk_size, user_stream, device_id)
{
  impl->core.set_policy(checksum_policy);
}
HCAMD_MANAGER_METHODS(SnappyManager)
CompressionConfig SnappyManager::configure_frame_compression(size_t n) { return impl->core.sz_configure_compression(n); }
CompressionConfig SnappyManager::configure_frame_compression(size_t n, SnappyFrameIndex index)
{
  return impl->core.sz_configure_compression(n, index == SnappyFrameIndex::Leading);
}
void SnappyManager::compress_frame(const uint8_t* in, uint8_t* frame, const CompressionConfig& c, size_t* frame_bytes,
                                   SnappyFrameIndex index)
{
  impl->core.sz_compress(in, frame, c, frame_bytes, index == SnappyFrameIndex::Leading);
}
size_t SnappyManager::get_frame_walked_chunks() { return impl->core.sz_walked_chunks(); }
void SnappyManager::decompress_frame_range(uint8_t* out, const uint8_t* frames, size_t frames_bytes, const DecompressionConfig& c,
                                           size_t first_byte, size_t num_bytes)
{
  impl->core.sz_decompress_range(out, frames, frames_bytes, c, first_byte, num_bytes);
}
void SnappyManager::get_parquet_pages_sizes(const uint8_t* const* device_chunk_ptrs, const size_t* device_chunk_bytes,
                                            size_t* device_num_pages, size_t* device_decompressed_bytes,
                                            hipcompStatus_t* device_statuses, size_t num_chunks, ParquetCodec codec)
{
  impl->core.pages_sizes(device_chunk_ptrs, device_chunk_bytes, device_num_pages, device_decompressed_bytes, device_statuses,
                         num_chunks, codec);
}
void SnappyManager::decompress_parquet_pages(const uint8_t* const* device_chunk_ptrs, const size_t* device_chunk_bytes,
                                             uint8_t* const* device_out_ptrs, const size_t* device_out_capacities,
                                             size_t* device_actual_bytes, hipcompStatus_t* device_statuses,
                                             ParquetPageInfo* const* device_page_ptrs, const size_t* device_page_capacities,
                                             size_t* device_num_pages, size_t num_chunks, ParquetCodec codec)
{
  impl->core.pages_call(device_chunk_ptrs, device_chunk_bytes, device_out_ptrs, device_out_capacities, device_actual_bytes,
                        device_statuses, device_page_ptrs, device_page_capacities, device_num_pages, num_chunks, codec);
}
void SnappyManager::set_parquet_pass_pages(size_t pages) { impl->core.pages_pass_limit = pages; }
ParquetPagesStats SnappyManager::get_parquet_pages_stats() const { return impl->core.pages_stats; }
void SnappyManager::compress_frame(const uint8_t* in, uint8_t* frame, const CompressionConfig& c, size_t* frame_bytes)
{
  impl->core.sz_compress(in, frame, c, frame_bytes);
}
DecompressionConfig SnappyManager::configure_frame_decompression(const uint8_t* frames, size_t frames_bytes)
{
  return impl->core.sz_configure_decompression(frames, frames_bytes);
}
void SnappyManager::decompress_frame(uint8_t* out, const uint8_t* frames, size_t frames_bytes, const DecompressionConfig& c)
{
  impl->core.sz_decompress(out, frames, frames_bytes, c);
}

// Every chunk of the container is one partition of the batched Cascaded codec, cut into the
// reference's 4096-byte sub-chunks whatever options.chunk_size says (that is the CONTAINER's
// chunk size here, as in the reference's CascadedManager.hpp:52-57), so the reference reads it.
CascadedManager::CascadedManager(const hipcompBatchedCascadedOpts_t& options, hipStream_t user_stream, int device_id)
{
  size_t slot = 0;
  if (options.chunk_size == 0
      || hipcompBatchedCascadedCompressGetMaxOutputChunkSize(options.chunk_size, hipcompBatchedCascadedDefaultOpts, &slot)
             != hipcompSuccess)
    throw std::runtime_error("CascadedManager: bad chunk size");
  size_t elem = 0;
  switch (options.type) {
  case HIPCOMP_TYPE_CHAR: case HIPCOMP_TYPE_UCHAR: elem = 1; break;
  case HIPCOMP_TYPE_SHORT: case HIPCOMP_TYPE_USHORT: elem = 2; break;
  case HIPCOMP_TYPE_INT: case HIPCOMP_TYPE_UINT: elem = 4; break;
  case HIPCOMP_TYPE_LONGLONG: case HIPCOMP_TYPE_ULONGLONG: elem = 8; break;
  default: throw std::runtime_error("CascadedManager: unsupported data type");
  }
  if (options.chunk_size % elem)
    throw std::runtime_error("CascadedManager: chunk_size must be a multiple of the element size");
  impl.reset(new Impl(options.chunk_size, user_stream, device_id));
  Core& m = impl->core;
  m.format = kCascaded;
  m.format_header_bytes = sizeof(CascadedFormatSpecHeader);
  static_assert(sizeof(CascadedFormatSpecHeader) <= kMaxFormatHeaderBytes, "format header");
  std::memcpy(m.format_header.bytes, &options, sizeof(options));
  m.cascaded_opts = options;
  m.cascaded_opts.chunk_size = 4096;
  m.cascaded_elem = (int)elem;
  m.place_align = 8;
  m.finish_init(slot);
}
CascadedManager::CascadedManager(const hipcompBatchedCascadedOpts_t& options, hipStream_t user_stream, int device_id,
                                 ChecksumPolicy checksum_policy)
    : CascadedManager(options, user_stream, device_id)
{
  impl->core.set_policy(checksum_policy);
}
HCAMD_MANAGER_METHODS(CascadedManager)
void CascadedManager::decode_parquet_hybrid(const uint8_t* const* device_stream_ptrs, const size_t* device_stream_bytes,
                                            const uint32_t* device_bit_widths, const size_t* device_num_values,
                                            void* const* device_out_ptrs, const size_t* device_out_capacities,
                                            size_t* device_consumed_bytes, const uint32_t* device_match_values,
                                            size_t* device_match_counts, hipcompStatus_t* device_statuses, size_t num_items,
                                            ParquetHybridForm form, hipcompType_t out_type)
{
  impl->core.hybrid_call(device_stream_ptrs, device_stream_bytes, device_bit_widths, device_num_values, device_out_ptrs,
                         device_out_capacities, device_consumed_bytes, device_match_values, device_match_counts, device_statuses,
                         num_items, form, out_type);
}
void CascadedManager::decode_parquet_delta(const uint8_t* const* device_stream_ptrs, const size_t* device_stream_bytes,
                                           const size_t* device_num_values, void* const* device_out_ptrs,
                                           const size_t* device_out_capacities, size_t* device_value_counts,
                                           size_t* device_consumed_bytes, hipcompStatus_t* device_statuses, size_t num_items,
                                           ParquetDeltaOutput output, hipcompType_t out_type)
{
  impl->core.delta_call(device_stream_ptrs, device_stream_bytes, device_num_values, device_out_ptrs, device_out_capacities,
                        device_value_counts, device_consumed_bytes, device_statuses, num_items, output, out_type);
}
void CascadedManager::index_parquet_dictionary(const uint8_t* const* device_dict_ptrs, const size_t* device_dict_bytes,
                                               const size_t* device_num_entries, int32_t* const* device_offset_ptrs,
                                               const size_t* device_offset_capacities, size_t* device_entry_counts,
                                               hipcompStatus_t* device_statuses, size_t num_dicts)
{
  impl->core.dict_index_call(device_dict_ptrs, device_dict_bytes, device_num_entries, device_offset_ptrs, device_offset_capacities,
                             device_entry_counts, device_statuses, num_dicts);
}
void CascadedManager::gather_parquet_dictionary(const uint8_t* const* device_dict_ptrs, const size_t* device_dict_bytes,
                                                const size_t* device_dict_entries, const uint32_t* const* device_index_ptrs,
                                                const size_t* device_num_indices, const uint8_t* const* device_level_ptrs,
                                                const size_t* device_num_rows, const uint32_t* device_max_levels,
                                                void* const* device_out_ptrs, const size_t* device_out_capacities,
                                                uint8_t* const* device_validity_ptrs, hipcompStatus_t* device_statuses,
                                                size_t num_items, uint32_t entry_bytes)
{
  impl->core.dict_gather_call(device_dict_ptrs, device_dict_bytes, device_dict_entries, device_index_ptrs, device_num_indices,
                              device_level_ptrs, device_num_rows, device_max_levels, device_out_ptrs, device_out_capacities,
                              device_validity_ptrs, device_statuses, num_items, entry_bytes);
}
void CascadedManager::gather_parquet_dictionary_strings(
    const uint8_t* const* device_dict_ptrs, const size_t* device_dict_bytes, const size_t* device_dict_entries,
    const int32_t* const* device_dict_offsets, const uint32_t* const* device_index_ptrs, const size_t* device_num_indices,
    const uint8_t* const* device_level_ptrs, const size_t* device_num_rows, const uint32_t* device_max_levels,
    int32_t* const* device_out_offsets, const size_t* device_offset_capacities, uint8_t* const* device_out_bytes,
    const size_t* device_byte_capacities, size_t* device_out_byte_counts, uint8_t* const* device_validity_ptrs,
    hipcompStatus_t* device_statuses, size_t num_items)
{
  impl->core.dict_strings_call(device_dict_ptrs, device_dict_bytes, device_dict_entries, device_dict_offsets, device_index_ptrs,
                               device_num_indices, device_level_ptrs, device_num_rows, device_max_levels, device_out_offsets,
                               device_offset_capacities, device_out_bytes, device_byte_capacities, device_out_byte_counts,
                               device_validity_ptrs, device_statuses, num_items);
}
void CascadedManager::place_parquet_values(const uint8_t* const* device_value_ptrs, const size_t* device_value_bytes,
                                           const size_t* device_value_starts, const size_t* device_num_values,
                                           const uint8_t* const* device_level_ptrs, const size_t* device_num_rows,
                                           const uint32_t* device_max_levels, void* const* device_out_ptrs,
                                           const size_t* device_out_capacities, uint8_t* const* device_validity_ptrs,
                                           hipcompStatus_t* device_statuses, size_t num_items, uint32_t value_bytes,
                                           ParquetValueLayout layout)
{
  impl->core.place_values_call(device_value_ptrs, device_value_bytes, device_value_starts, device_num_values, device_level_ptrs,
                               device_num_rows, device_max_levels, device_out_ptrs, device_out_capacities, device_validity_ptrs,
                               device_statuses, num_items, value_bytes, layout);
}
void CascadedManager::place_parquet_booleans(const uint8_t* const* device_value_ptrs, const size_t* device_value_bytes,
                                             const size_t* device_value_starts, const size_t* device_num_values,
                                             const uint8_t* const* device_level_ptrs, const size_t* device_num_rows,
                                             const uint32_t* device_max_levels, uint8_t* const* device_out_ptrs,
                                             const size_t* device_out_capacities, uint8_t* const* device_validity_ptrs,
                                             hipcompStatus_t* device_statuses, size_t num_items)
{
  impl->core.place_booleans_call(device_value_ptrs, device_value_bytes, device_value_starts, device_num_values, device_level_ptrs,
                                 device_num_rows, device_max_levels, device_out_ptrs, device_out_capacities, device_validity_ptrs,
                                 device_statuses, num_items);
}
void CascadedManager::place_parquet_strings(const uint8_t* const* device_body_ptrs, const size_t* device_body_bytes,
                                            const size_t* device_value_starts, const int32_t* const* device_value_offsets,
                                            const size_t* device_num_values, const uint8_t* const* device_level_ptrs,
                                            const size_t* device_num_rows, const uint32_t* device_max_levels,
                                            int32_t* const* device_out_offsets, const size_t* device_offset_capacities,
                                            uint8_t* const* device_out_bytes, const size_t* device_byte_capacities,
                                            size_t* device_out_byte_counts, uint8_t* const* device_validity_ptrs,
                                            hipcompStatus_t* device_statuses, size_t num_items, ParquetStringLayout layout)
{
  impl->core.place_strings_call(device_body_ptrs, device_body_bytes, device_value_starts, device_value_offsets, device_num_values,
                                device_level_ptrs, device_num_rows, device_max_levels, device_out_offsets, device_offset_capacities,
                                device_out_bytes, device_byte_capacities, device_out_byte_counts, device_validity_ptrs,
                                device_statuses, num_items, layout);
}

// reference hipcompManagerFactory.cpp:44-148 (synchronises the stream, as there)
std::shared_ptr<hipcompManagerBase> create_manager(const uint8_t* comp_buffer, hipStream_t stream, const int device_id)
{
  return create_manager(comp_buffer, stream, device_id, NoComputeNoVerify);
}

std::shared_ptr<hipcompManagerBase> create_manager(
    const uint8_t* comp_buffer, hipStream_t stream, const int device_id, ChecksumPolicy checksum_policy)
{
  struct Heads
  {
    CommonHeader common;
    FormatHeader format;
  } heads;
  check(hipMemcpyAsync(&heads, comp_buffer, sizeof(heads), hipMemcpyDeviceToHost, stream), "create_manager: read headers");
  check(hipStreamSynchronize(stream), "create_manager: read headers");
  switch (heads.common.format) {
  case kLZ4: {
    uint32_t t;
    std::memcpy(&t, heads.format.bytes, sizeof(t));
    return std::make_shared<LZ4Manager>((size_t)heads.common.uncomp_chunk_size, (hipcompType_t)t, stream, device_id,
                                        checksum_policy);
  }
  case kSnappy:
    return std::make_shared<SnappyManager>((size_t)heads.common.uncomp_chunk_size, stream, device_id, checksum_policy);
  case kCascaded: {
    hipcompBatchedCascadedOpts_t o;
    std::memcpy(&o, heads.format.bytes, sizeof(o));
    if (o.chunk_size != heads.common.uncomp_chunk_size)
      throw std::runtime_error("create_manager: Cascaded options do not match the container's chunk size");
    return std::make_shared<CascadedManager>(o, stream, device_id, checksum_policy);
  }
  default:
    throw std::runtime_error("create_manager: format " + std::to_string((int)heads.common.format)
                             + " is not supported (LZ4, Snappy and Cascaded are)");
  }
}

} // namespace hipcomp

// ---- C binding -----------------------------------------------------------------------------
struct hipcompHlifManager
{
  std::shared_ptr<hipcomp::hipcompManagerBase> lz4; // (any of the managers)
  hipStream_t stream = nullptr;
  std::unique_ptr<hipcomp::CompressionConfig> last_comp;
  std::unique_ptr<hipcomp::DecompressionConfig> last_decomp;
  bool last_was_compress = true;
};

namespace {
template <typename F>
hipcompStatus_t guarded(const char* fn, F&& f)
{
  try {
    f();
    return hipcompSuccess;
  } catch (const std::exception& e) {
    return hcamd::fail(fn, e.what());
  }
}
} // namespace

extern "C" {

hipcompStatus_t hipcompHlifLZ4ManagerCreate(
    size_t uncomp_chunk_size, hipcompType_t data_type, hipStream_t stream, hipcompHlifManager_t** manager)
{
  static const char* fn = "hipcompHlifLZ4ManagerCreate()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  return guarded(fn, [&] {
    int dev = 0;
    hcamd::hlif::check(hipGetDevice(&dev), "hipGetDevice");
    std::unique_ptr<hipcompHlifManager> h(new hipcompHlifManager);
    h->lz4 = std::make_shared<hipcomp::LZ4Manager>(uncomp_chunk_size, data_type, stream, dev);
    h->stream = stream;
    *manager = h.release();
  });
}

hipcompStatus_t hipcompHlifSnappyManagerCreate(size_t uncomp_chunk_size, hipStream_t stream, hipcompHlifManager_t** manager)
{
  static const char* fn = "hipcompHlifSnappyManagerCreate()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  return guarded(fn, [&] {
    int dev = 0;
    hcamd::hlif::check(hipGetDevice(&dev), "hipGetDevice");
    std::unique_ptr<hipcompHlifManager> h(new hipcompHlifManager);
    h->lz4 = std::make_shared<hipcomp::SnappyManager>(uncomp_chunk_size, stream, dev);
    h->stream = stream;
    *manager = h.release();
  });
}

hipcompStatus_t hipcompHlifCascadedManagerCreate(
    hipcompBatchedCascadedOpts_t options, hipStream_t stream, hipcompHlifManager_t** manager)
{
  static const char* fn = "hipcompHlifCascadedManagerCreate()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  return guarded(fn, [&] {
    int dev = 0;
    hcamd::hlif::check(hipGetDevice(&dev), "hipGetDevice");
    std::unique_ptr<hipcompHlifManager> h(new hipcompHlifManager);
    h->lz4 = std::make_shared<hipcomp::CascadedManager>(options, stream, dev);
    h->stream = stream;
    *manager = h.release();
  });
}

hipcompStatus_t hipcompHlifManagerCreateFromContainer(
    const void* device_container, hipStream_t stream, hipcompHlifManager_t** manager)
{
  static const char* fn = "hipcompHlifManagerCreateFromContainer()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, device_container);
  return guarded(fn, [&] {
    int dev = 0;
    hcamd::hlif::check(hipGetDevice(&dev), "hipGetDevice");
    std::unique_ptr<hipcompHlifManager> h(new hipcompHlifManager);
    h->lz4 = hipcomp::create_manager(static_cast<const uint8_t*>(device_container), stream, dev);
    h->stream = stream;
    *manager = h.release();
  });
}

hipcompStatus_t hipcompHlifManagerDestroy(hipcompHlifManager_t* manager)
{
  delete manager;
  return hipcompSuccess;
}

hipcompStatus_t hipcompHlifConfigureCompression(
    hipcompHlifManager_t* manager, size_t uncompressed_bytes, size_t* max_compressed_bytes, size_t* num_chunks)
{
  static const char* fn = "hipcompHlifConfigureCompression()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, max_compressed_bytes);
  return guarded(fn, [&] {
    const hipcomp::CompressionConfig c = manager->lz4->configure_compression(uncompressed_bytes);
    *max_compressed_bytes = c.max_compressed_buffer_size;
    if (num_chunks)
      *num_chunks = c.num_chunks;
  });
}

hipcompStatus_t hipcompHlifCompress(
    hipcompHlifManager_t* manager, const void* device_uncompressed, size_t uncompressed_bytes, void* device_container)
{
  static const char* fn = "hipcompHlifCompress()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, device_container);
  return guarded(fn, [&] {
    // (a configuration owns a pinned status word: made anew only when the size changes -- hipHostMalloc /
    // hipHostFree per call were a fifth of a 3 ms compress)
    if (!manager->last_comp || manager->last_comp->uncompressed_buffer_size != uncompressed_bytes)
      manager->last_comp.reset(new hipcomp::CompressionConfig(manager->lz4->configure_compression(uncompressed_bytes)));
    manager->last_was_compress = true;
    manager->lz4->compress(static_cast<const uint8_t*>(device_uncompressed), static_cast<uint8_t*>(device_container),
                           *manager->last_comp);
  });
}

hipcompStatus_t hipcompHlifGetDecompressedSize(
    hipcompHlifManager_t* manager, const void* device_container, size_t* uncompressed_bytes, size_t* num_chunks)
{
  static const char* fn = "hipcompHlifGetDecompressedSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, device_container);
  HCAMD_REQUIRE_NOT_NULL(fn, uncompressed_bytes);
  return guarded(fn, [&] {
    const hipcomp::DecompressionConfig d = manager->lz4->configure_decompression(static_cast<const uint8_t*>(device_container));
    *uncompressed_bytes = d.decomp_data_size;
    if (num_chunks)
      *num_chunks = d.num_chunks;
  });
}

hipcompStatus_t hipcompHlifGetCompressedSize(
    hipcompHlifManager_t* manager, const void* device_container, size_t* container_bytes)
{
  static const char* fn = "hipcompHlifGetCompressedSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, device_container);
  HCAMD_REQUIRE_NOT_NULL(fn, container_bytes);
  return guarded(fn, [&] {
    *container_bytes = manager->lz4->get_compressed_output_size(static_cast<uint8_t*>(const_cast<void*>(device_container)));
  });
}

hipcompStatus_t hipcompHlifDecompress(hipcompHlifManager_t* manager, const void* device_container, void* device_uncompressed)
{
  static const char* fn = "hipcompHlifDecompress()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, device_container);
  return guarded(fn, [&] {
    manager->last_decomp.reset(new hipcomp::DecompressionConfig(
        manager->lz4->configure_decompression(static_cast<const uint8_t*>(device_container))));
    manager->last_was_compress = false;
    manager->lz4->decompress(static_cast<uint8_t*>(device_uncompressed), static_cast<const uint8_t*>(device_container),
                             *manager->last_decomp);
  });
}

hipcompStatus_t hipcompHlifGetLastStatus(hipcompHlifManager_t* manager, hipcompStatus_t* status)
{
  static const char* fn = "hipcompHlifGetLastStatus()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, status);
  return guarded(fn, [&] {
    hcamd::hlif::check(hipStreamSynchronize(manager->stream), "hipStreamSynchronize");
    *status = hipcompSuccess;
    if (manager->last_was_compress && manager->last_comp)
      *status = *manager->last_comp->get_status();
    if (!manager->last_was_compress && manager->last_decomp)
      *status = *manager->last_decomp->get_status();
  });
}

hipcompStatus_t hipcompHlifGetRequiredScratchBytes(hipcompHlifManager_t* manager, size_t* scratch_bytes)
{
  static const char* fn = "hipcompHlifGetRequiredScratchBytes()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, scratch_bytes);
  *scratch_bytes = manager->lz4->get_required_scratch_buffer_size();
  return hipcompSuccess;
}

hipcompStatus_t hipcompHlifSetScratchBuffer(hipcompHlifManager_t* manager, void* device_scratch)
{
  static const char* fn = "hipcompHlifSetScratchBuffer()";
  HCAMD_REQUIRE_NOT_NULL(fn, manager);
  HCAMD_REQUIRE_NOT_NULL(fn, device_scratch);
  manager->lz4->set_scratch_buffer(static_cast<uint8_t*>(device_scratch));
  return hipcompSuccess;
}

} // extern "C"
