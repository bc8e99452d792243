// checksum_launch.hpp -- host-callable launchers of the CRC-32 kernels of the high-level managers
// (checksum_kernels.hip; the definition and the algebra: crc32_math.hpp).
//
// A manager's compress or decompress runs in passes of up to Core::kPlacedSlab chunks (hlif.hip).  Per pass
// the chunk CRC kernel computes one CRC per chunk of a list, writes it (compute) or compares it with the
// container's (verify), and XORs crc32_shift(crc_i, bytes of the pass behind chunk i) into the pass word of its
// side.  The fold kernel then joins the pass to the passes before it (acc = shift(acc, pass bytes) ^ pass
// word), so that the full checksums come out in chunk-index order whatever order the chunks were placed in.
// Where the chunks of a pass are not all chunk_bytes long (the compressed side), the scan kernels give the
// bytes in front of each chunk first.  Everything is stream-ordered: no host synchronisation.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"

namespace hcamd {

// the checksum state of one compress or decompress call (device memory, in the manager's scratch)
struct CrcState
{
  uint32_t comp_acc, decomp_acc;   // full checksums of the passes so far
  uint32_t comp_pass, decomp_pass; // this pass's XOR sums
  uint64_t comp_pass_bytes;        // compressed bytes of this pass (the scan's total)
  uint32_t flags;                  // kCrcBad | kCrcNoHeader
  uint32_t pad;
};
constexpr uint32_t kCrcBad = 1;      // a stored value differs
constexpr uint32_t kCrcNoHeader = 2; // the header check failed: no chunk was read, nothing compared
// device bytes the checksums of a pass of `chunks` chunks need besides the state (the scan's output)
constexpr size_t crc_pass_bytes(size_t chunks) { return 8 * chunks + 8 * ((chunks + 1023) / 1024) + 64; }

// one side of a pass: the chunks ...
struct CrcChunks
{
  const uint8_t* const* ptrs = nullptr;        // chunk i at ptrs[i], or (ptrs == nullptr) at base + offsets[i]
  const uint8_t* base = nullptr;
  const unsigned long long* offsets = nullptr;
  const size_t* lens = nullptr;                // its bytes
  const size_t* caps = nullptr;                // nullptr, or: caps[i] == 0 means the header check failed (no bytes
                                               // are read, nothing is compared) ...
  bool clamp_to_caps = false;                  // ... and, if set, chunk i has min(lens[i], caps[i]) bytes
  uint32_t count = 0;
};
// ... and what becomes of their CRCs
struct CrcTarget
{
  uint32_t* values = nullptr;         // compute: values[i] = CRC of chunk i
  const uint32_t* stored = nullptr;   // verify: compared with stored[i]
  const bool* present = nullptr;      // verify: the container's flag; false: nothing is read or checked
  const uint64_t* before = nullptr;   // bytes of the pass in front of chunk i: before[i] + before[count + i / 1024]
                                      // (crc_launch_scan's output), or nullptr: i * stride
  uint64_t stride = 0;
  const uint64_t* pass_bytes_dev = nullptr; // bytes of the pass (a device word), or nullptr: pass_bytes
  uint64_t pass_bytes = 0;
  uint32_t* pass_word = nullptr;
  uint32_t* flags = nullptr;
};

hipError_t crc_launch_reset(CrcState* st, hipStream_t stream);
// The bytes in front of each chunk of the list (lens as CrcChunks reads them), in two parts: work[i] from the
// start of i's group of 1024 chunks, work[count + g] in front of group g; st->comp_pass_bytes = all of them.
// `work` = crc_pass_bytes(count) bytes of scratch.  count <= 1024 * 1024.
hipError_t crc_launch_scan(const CrcChunks& c, uint64_t* work, CrcState* st, hipStream_t stream);
hipError_t crc_launch_chunks(const CrcChunks& c, const CrcTarget& t, hipStream_t stream);
// acc = shift(acc, pass bytes) ^ pass word, pass words = 0 (decomp_pass_bytes: host-known)
hipError_t crc_launch_fold(CrcState* st, uint64_t decomp_pass_bytes, hipStream_t stream);
// compress: the full checksums into the header, both per-chunk flags true
hipError_t crc_launch_finish_compress(uint32_t* full_comp, uint32_t* full_decomp, bool* comp_flag, bool* decomp_flag,
                                      const CrcState* st, hipStream_t stream);
// decompress: the full checksums checked where the flags say they are present, then the status:
// BadChecksum > CannotDecompress > CannotVerifyChecksums (when `require` and a flag is false) > Success
hipError_t crc_launch_finish_decompress(const uint32_t* full_comp, const uint32_t* full_decomp, const bool* comp_flag,
                                        const bool* decomp_flag, const CrcState* st, bool require,
                                        hipcompStatus_t* status, hipStream_t stream);

} // namespace hcamd
