/*
 * hipcomp/hipcompManager.hpp -- the high-level interface ("HLIF"): one call compresses a
 * whole device buffer into ONE self-describing container, one call decompresses it.
 *
 * Same public surface as the reference (include/hipcomp/hipcompManager.hpp:50-303):
 * CompressionConfig / DecompressionConfig with the same public fields and get_status(),
 * hipcompManagerBase with the same eight virtuals; same container layout
 * (src/hipcomp_common_deps/hlif_shared_types.hpp:68-84, src/highlevel/BatchManager.hpp:
 * 108-112, 245-251), so a container written here is read by the reference's managers and
 * the other way round:
 *
 *   CommonHeader (64 B) | format header | pad to 8 | chunk offsets u64 x n |
 *   chunk sizes u64 x n | 2 x checksums u32 x n (zero unless a ChecksumPolicy computes them) | chunk data
 *
 * Behind it are the batched codecs of this library (the chunks of a container are exactly
 * the streams hipcompBatched*CompressAsync produces).  Differences by design: chunk data
 * lies in chunk order (the reference places chunks in completion order; both record the
 * offsets), configs own their status word instead of borrowing it from a pool, and
 * max_compressed_buffer_size counts the size array at its true width.
 *
 * Ranged reads.  The three managers (lz4.hpp, snappy.hpp, cascaded.hpp) also have a non-virtual
 *
 *   void decompress_range(uint8_t* out, const uint8_t* comp_buffer, const DecompressionConfig& cfg,
 *                         size_t first_byte, size_t num_bytes);
 *
 * which writes bytes [first_byte, first_byte + num_bytes) of the uncompressed buffer to out[0, num_bytes) and
 * no byte outside that span, at any alignment of out.  cfg comes from either configure_decompression.  Like
 * decompress it is asynchronous on the manager's stream and leaves its status in cfg.get_status():
 * hipcompErrorInvalidValue when first_byte + num_bytes overflows or exceeds cfg.decomp_data_size (CascadedManager:
 * also when either is not a multiple of the element size) -- nothing else is launched --, otherwise decompress's
 * BadChecksum > CannotDecompress > CannotVerifyChecksums > Success.  Only the chunks the range touches are read,
 * decoded and, under a verifying policy, checked against their per-chunk checksums (the chunks at the range's ends
 * are decoded whole into scratch space, so they are checked too); the two full-buffer checksums are not checked.
 * A chunk that fails leaves its part of out as it was.  The scratch space is the manager's
 * (get_required_scratch_buffer_size() is what it was).  INTEGRATION.md has the contract in full.
 *
 * Reading many ranges.  The three managers also have a non-virtual
 *
 *   void decompress_ranges(uint8_t* out, size_t out_bytes, const uint8_t* comp_buffer, const DecompressionConfig& cfg,
 *                          const size_t* device_first_bytes, const size_t* device_num_bytes, size_t num_ranges,
 *                          size_t* device_out_offsets);   // may be null; num_ranges + 1 entries
 *
 * for the rows a filter selected or the values behind a list of offsets.  The two range arrays lie in device
 * memory and the host never reads them.  Range r is bytes [first[r], first[r] + num[r]) of the uncompressed
 * buffer; the ranges land in out back to back in the order given, range r at off[r], the exclusive sum of the
 * lengths in front of it, and where device_out_offsets is given off[0 .. num_ranges] is written there (the last
 * entry: the total).  Ranges may be empty, overlap, repeat and come in any order; out may lie at any alignment.
 * A range decompress_range would refuse, or a total above out_bytes, refuses the whole call:
 * hipcompErrorInvalidValue, no byte of out or of device_out_offsets written (the decision is a word on the
 * device).  A header that contradicts cfg: hipcompErrorCannotDecompress, nothing written either.  Every chunk
 * some range touches is decoded once per call, whole, into scratch space and, under a verifying policy, checked on
 * both sides once; the status is decompress_range's.  A chunk that fails gives nothing to the ranges that touch
 * it (their bytes are unspecified but inside out[0, total)); every other range holds exactly its bytes.
 * num_ranges == 0 is success and launches nothing.  Otherwise the call synchronises the stream ONCE, after its
 * plan, to learn how many passes to enqueue: it cannot be captured into a graph.  The scratch space is the
 * manager's (get_required_scratch_buffer_size() is what it was) and also holds the call's tables, about
 * 12 bytes per range and a byte per 4 chunks; a scratch that cannot hold them and two chunks makes the call throw.
 *
 *   size_t get_ranges_pass_chunks() const;   // distinct chunks one pass decodes with the scratch the manager has
 *                                            // now (before a call's tables take their share of a caller's buffer)
 *   RangesStats get_ranges_stats() const;    // of the last call: what its one synchronisation fetched
 *
 * There is no such call for frames and no C binding.  It is built for many small ranges; for a few large ones
 * decompress_range, which decodes interior chunks straight into out, stays the better call.
 */
#ifndef HIPCOMP_MANAGER_HPP
#define HIPCOMP_MANAGER_HPP

#include "hipcomp.h"

#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include <memory>

namespace hipcomp
{

/* What a manager does with the CRC-32 checksums of its containers (nvCOMP 3's names; INTEGRATION.md says what
   each checksum covers).  Compute*: compress fills the header's two full checksums and both per-chunk arrays
   and sets both include_per_chunk_* flags.  *Verify*: decompress checks what the container's flags say is
   present and reports hipcompErrorBadChecksum when a stored value differs; ComputeAndVerify also reports
   hipcompErrorCannotVerifyChecksums when a flag is false.  The constructors without a policy mean
   NoComputeNoVerify: containers as the reference writes them (zeros, false), nothing checked. */
enum ChecksumPolicy
{
  NoComputeNoVerify,
  ComputeAndNoVerify,
  NoComputeAndVerifyIfPresent,
  ComputeAndVerifyIfPresent,
  ComputeAndVerify
};

struct CompressionConfig
{
  size_t uncompressed_buffer_size;
  size_t max_compressed_buffer_size;
  size_t num_chunks;
  explicit CompressionConfig(size_t uncompressed_buffer_size);
  /* the status word of the operation: pinned host memory the device writes (read it after
     synchronising the stream) */
  hipcompStatus_t* get_status() const;

private:
  std::shared_ptr<hipcompStatus_t> status;
};

struct DecompressionConfig
{
  size_t decomp_data_size;
  uint32_t num_chunks;
  DecompressionConfig();
  hipcompStatus_t* get_status() const;

private:
  std::shared_ptr<hipcompStatus_t> status;
};

/* what the last decompress_ranges of a manager found (host values, no synchronisation): the ranges it was given,
   the distinct chunks they touch (each decoded once), the passes that took, the sum of the lengths.  A refused
   call, or one whose header check failed, has 0 touched chunks and 0 passes. */
struct RangesStats
{
  size_t ranges;
  size_t touched_chunks;
  size_t passes;
  size_t total_bytes;
};

struct hipcompManagerBase
{
  /* sizes the result buffer for an input of decomp_buffer_size bytes */
  virtual CompressionConfig configure_compression(const size_t decomp_buffer_size) = 0;
  /* asynchronous on the manager's stream; both buffers device-accessible */
  virtual void compress(const uint8_t* decomp_buffer, uint8_t* comp_buffer, const CompressionConfig& comp_config) = 0;
  /* reads the container's header (synchronises the stream); the status (after decompress) is
     hipcompErrorBadChecksum > hipcompErrorCannotDecompress > hipcompErrorCannotVerifyChecksums > hipcompSuccess */
  virtual DecompressionConfig configure_decompression(const uint8_t* comp_buffer) = 0;
  /* from the config the buffer was compressed with (no synchronisation) */
  virtual DecompressionConfig configure_decompression(const CompressionConfig& comp_config) = 0;
  virtual void decompress(uint8_t* decomp_buffer, const uint8_t* comp_buffer, const DecompressionConfig& decomp_config) = 0;
  /* the manager allocates its scratch space on first use unless one is set */
  virtual void set_scratch_buffer(uint8_t* new_scratch_buffer) = 0;
  virtual size_t get_required_scratch_buffer_size() = 0;
  /* bytes of the container at comp_buffer (copies its header to the host) */
  virtual size_t get_compressed_output_size(uint8_t* comp_buffer) = 0;
  virtual ~hipcompManagerBase() = default;
};

} // namespace hipcomp

#endif
