// zstd_kernels.hip -- batched Zstandard (RFC 8878) decoder for gfx950, one chunk per wavefront.
//
// Shape:
//   * kWavesPerBlock waves per workgroup, each with its own slice of LDS and its own literal buffer in the temp
//     space; the waves share nothing and never meet at a barrier.  Chunks are taken grid-stride.
//   * Headers, table descriptions and the sequence bitstream are wave-uniform: every byte is loaded at a uniform
//     address and moved to a scalar register (UBytes), the backward bitstream keeps a 64-bit window there, the
//     three FSE states and the repeat offsets are scalars.  The format logic is zstd_tables.hpp, the same
//     functions the CPU driver composes.
//   * Literals: raw literals are read where they lie, RLE literals are a 64-lane fill of the wave's literal
//     buffer, Huffman literals are walked by lanes 0-3, one stream each, every lane storing its own bytes.
//   * Sequences are decoded 64 at a time, sequence k handed to lane k.  Two DPP prefix sums give every literal
//     run's source and destination; all runs of the batch are then copied in one trip in which each lane finds
//     its run by a search over the prefix sums.  The matches follow in order, each a 64-lane copy that reads its
//     source modulo the offset where it overlaps itself.
//   * Every path checks its bounds first; a chunk that breaks one ends with hipcompErrorCannotDecompress and
//     nothing is read or written outside the chunk's two ranges and the wave's literal buffer.
#include <hip/hip_runtime.h>

#include "wave_utils.hpp"
#include "zstd_launch.hpp"
#include "zstd_tables.hpp"

namespace hcamd {
namespace {

using namespace zstd;

struct WaveLds
{
  FseEntry ll[1 << kLLLogMax], ml[1 << kMLLogMax], of[1 << kOFLogMax], wt[1 << kWeightLogMax];
  uint16_t huf[1 << kHufLogMax];
  int16_t norm[256];
  uint16_t next[256];
  uint8_t weights[256], sorted[256];
  uint32_t hcount[16];
  uint32_t lit_end[kWave], lit_shift[kWave];
};
static_assert(sizeof(WaveLds) <= kLdsPerWave, "the per-wave LDS of zstd_sizing.hpp");

__device__ __forceinline__ void lds_phase() { lds_lane_exchange_fence(); }

// bytes of global memory at wave-uniform addresses, each moved to a scalar register
struct UBytes
{
  cgptr p;
  __device__ __forceinline__ uint8_t operator[](uint64_t i) const { return (uint8_t)uniform((uint32_t)p[i]); }
  __device__ __forceinline__ UBytes operator+(uint64_t i) const { return UBytes{p + i}; }
};

// an FSE table in LDS read at a wave-uniform state
struct UTable
{
  const FseEntry* t;
  __device__ __forceinline__ FseEntry operator[](uint32_t i) const
  {
    const uint32_t v = uniform(*reinterpret_cast<const uint32_t*>(t + i));
    return FseEntry{(uint16_t)(v & 0xFFFFu), (uint8_t)((v >> 16) & 0xFFu), (uint8_t)(v >> 24)};
  }
};

struct Entropy
{
  uint32_t ll_log, of_log, ml_log, huf_log;
  bool have_huf, have_fse;
};

__device__ __forceinline__ bool seq_table(
    uint32_t mode, UBytes p, uint32_t n, uint32_t& at, FseEntry* table, uint32_t& log, const int16_t* def, uint32_t def_syms,
    uint32_t def_log, uint32_t max_sym, uint32_t max_log, bool have_previous, WaveLds& lds)
{
  if (mode == kPredefined) {
    for (uint32_t s = 0; s < def_syms; ++s)
      lds.norm[s] = def[s];
    fse_build(lds.norm, def_syms, def_log, table, lds.next);
    log = def_log;
    return true;
  }
  if (mode == kRleMode) {
    if (at >= n)
      return false;
    const uint32_t sym = p[at];
    if (sym > max_sym)
      return false;
    fse_build_rle(table, sym);
    log = 0;
    at += 1;
    return true;
  }
  if (mode == kFseMode) {
    const NCount nc = read_ncount(p + at, n - at, lds.norm, max_sym, max_log);
    if (!nc.ok)
      return false;
    fse_build(lds.norm, nc.nsym, nc.log, table, lds.next);
    log = nc.log;
    at += nc.bytes;
    return true;
  }
  return have_previous;
}

// `streams` (1 or 4) Huffman streams at src[0, n) -> lit[0, regen), lane j walking stream j
template <bool STORE>
__device__ __forceinline__ bool huf_literals(
    cgptr src, uint32_t n, uint32_t streams, gptr lit, uint32_t regen, const WaveLds& lds, uint32_t log, int lane)
{
  uint32_t size[4] = {n, 0, 0, 0};
  uint32_t seg = regen, first = 0;
  if (streams == 4u) {
    if (!huf_jump_table(UBytes{src}, n, size))
      return false;
    seg = (regen + 3u) / 4u;
    if (3u * seg > regen)
      return false;
    first = 6;
  }
  // this lane's stream: its bytes, its share of the literals
  uint32_t my_at = first, my_n = 0, my_count = 0;
  const bool active = (uint32_t)lane < streams;
  if (active) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < lane)
        my_at += size[j];
      if (j == lane)
        my_n = size[j];
    }
    my_count = streams == 1u ? regen : (lane < 3 ? seg : regen - 3u * seg);
  }
  BackBits<cgptr> bs{};
  bool good = true;
  if (active)
    good = bs.init(src + my_at, my_n);
  const uint32_t my_first = (uint32_t)lane * seg;
  if (active && good) {
    for (uint32_t i = 0; i < my_count; ++i) {
      const uint32_t e = lds.huf[bs.peek(log)];
      bs.left -= (int32_t)(e & 0xFFu);
      if (bs.left < 0)
        break;
      if (STORE)
        lit[my_first + i] = (uint8_t)(e >> 8);
    }
    good = bs.left == 0;
  }
  return wave_ballot(!good) == 0;
}

template <bool WRITE_OUT>
__device__ __forceinline__ bool decode_block(
    cgptr blk, uint32_t n, gptr out, uint64_t cap, uint64_t frame_start, uint64_t& outpos, gptr lit, uint64_t lit_cap,
    WaveLds& lds, Entropy& en, SeqState& st, int lane)
{
  const UBytes p{blk};
  const LitHeader lh = parse_literals_header(p, n);
  if (!lh.ok)
    return false;
  cgptr lits = static_cast<cgptr>(lit);
  cgptr body = blk + lh.header_bytes;
  if (lh.type == kRawLit) {
    lits = body; // read where they lie
  } else {
    if (WRITE_OUT && lh.regen > lit_cap)
      return false;
    if (lh.type == kRleLit) {
      if (WRITE_OUT) {
        const uint8_t v = p[lh.header_bytes];
        for (uint32_t i = (uint32_t)lane; i < lh.regen; i += kWave)
          lit[i] = v;
      }
    } else {
      uint32_t at = 0;
      if (lh.type == kHufLit) {
        const HufDesc d = read_huf_weights(UBytes{body}, lh.comp, lds.weights, lds.norm, lds.wt, lds.next);
        if (!d.ok)
          return false;
        huf_sort(lds.weights, d.nsym, lds.hcount, lds.sorted);
        lds_phase();
        for (uint32_t e = (uint32_t)lane; e < (1u << d.log); e += kWave)
          lds.huf[e] = (uint16_t)huf_entry(e, lds.hcount, lds.sorted, d.log);
        lds_phase();
        en.huf_log = d.log;
        en.have_huf = true;
        at = d.bytes;
      } else if (!en.have_huf) {
        return false;
      }
      if (!huf_literals<WRITE_OUT>(body + at, lh.comp - at, lh.streams, lit, lh.regen, lds, en.huf_log, lane))
        return false;
    }
  }
  const uint32_t lit_bytes = lh.header_bytes + lh.comp;
  const SeqHeader sh = parse_sequences_header(p + lit_bytes, n - lit_bytes);
  if (!sh.ok)
    return false;
  uint32_t at = lit_bytes + sh.header_bytes;
  uint32_t litpos = 0;
  if (sh.nseq) {
    if (!seq_table(sh.ll_mode, p, n, at, lds.ll, en.ll_log, kLLDefault, 36, kLLDefaultLog, kLLSymMax, kLLLogMax, en.have_fse, lds) ||
        !seq_table(sh.of_mode, p, n, at, lds.of, en.of_log, kOFDefault, 29, kOFDefaultLog, kOFSymMax, kOFLogMax, en.have_fse, lds) ||
        !seq_table(sh.ml_mode, p, n, at, lds.ml, en.ml_log, kMLDefault, 53, kMLDefaultLog, kMLSymMax, kMLLogMax, en.have_fse, lds))
      return false;
    en.have_fse = true;
    lds_phase();
    BackBits<UBytes> bs{};
    if (!bs.init(p + at, n - at))
      return false;
    st.ll = bs.read(en.ll_log);
    st.of = bs.read(en.of_log);
    st.ml = bs.read(en.ml_log);
    if (bs.left < 0)
      return false;
    const UTable llt{lds.ll}, oft{lds.of}, mlt{lds.ml};
    for (uint32_t done = 0; done < sh.nseq;) {
      const uint32_t m = sh.nseq - done < (uint32_t)kWave ? sh.nseq - done : (uint32_t)kWave;
      uint32_t my_ll = 0, my_ml = 0, my_off = 0;
      for (uint32_t k = 0; k < m; ++k) {
        const Sequence q = decode_sequence(bs, st, llt, oft, mlt, done + k + 1u == sh.nseq);
        if (bs.left < 0)
          return false;
        if ((uint32_t)lane == k) {
          my_ll = q.ll;
          my_ml = q.ml;
          my_off = q.off;
        }
      }
      // where every literal run and every match of the batch goes (each sum stays below 2^25)
      const uint32_t sum_ll = wave_scan_add_u32(my_ll);
      const uint32_t sum_all = wave_scan_add_u32(my_ll + my_ml);
      const uint32_t lit_total = read_lane(sum_ll, kWave - 1), out_total = read_lane(sum_all, kWave - 1);
      if (lit_total > lh.regen - litpos || out_total > cap - outpos)
        return false;
      const uint32_t match_dst = sum_all - my_ml; // from outpos
      if (wave_ballot((uint64_t)my_off > (outpos - frame_start) + match_dst) != 0)
        return false;
      if (WRITE_OUT) {
        lds_phase();
        lds.lit_end[lane] = sum_ll;
        lds.lit_shift[lane] = sum_all - my_ml - sum_ll; // literal i of the batch goes to outpos + i + shift of its run
        lds_phase();
        for (uint32_t i = (uint32_t)lane; i < lit_total; i += kWave) {
          uint32_t k = 0;
#pragma unroll
          for (uint32_t s = 32; s >= 1u; s >>= 1)
            if (lds.lit_end[k + s - 1u] <= i)
              k += s;
          out[outpos + i + lds.lit_shift[k]] = lits[litpos + i];
        }
        lds_phase();
        for (uint32_t k = 0; k < m; ++k) {
          const uint32_t ml = read_lane(my_ml, (int)k), off = read_lane(my_off, (int)k);
          gptr dst = out + (outpos + read_lane(match_dst, (int)k));
          cgptr src = static_cast<cgptr>(dst) - off;
          if (off >= (uint32_t)kWave || off >= ml) {
            // every 64-byte step reads bytes stored before it began
            for (uint32_t i = (uint32_t)lane; i < ml; i += kWave)
              dst[i] = src[i];
          } else {
            // the match runs into its own output: its source repeats with period `off`
            for (uint32_t i = (uint32_t)lane; i < ml; i += kWave)
              dst[i] = src[i % off];
          }
        }
      }
      litpos += lit_total;
      outpos += out_total;
      done += m;
    }
    if (bs.left != 0)
      return false;
  }
  const uint32_t tail = lh.regen - litpos;
  if (tail > cap - outpos)
    return false;
  if (WRITE_OUT) {
    for (uint32_t i = (uint32_t)lane; i < tail; i += kWave)
      out[outpos + i] = lits[litpos + i];
  }
  outpos += tail;
  return true;
}

// XXH64, seed 0, of out[0, n): lanes 0-3 hold one accumulator each (the other lanes repeat them)
__device__ __forceinline__ uint64_t xxh64_wave(cgptr out, uint64_t n, int lane)
{
  uint64_t h = kXxhP5;
  const uint64_t stripes = n >> 5;
  if (stripes) {
    const uint32_t j = (uint32_t)lane & 3u;
    uint64_t acc = xxh64_acc_init(j, 0);
    cgptr q = out + 8u * j;
    for (uint64_t s = 0; s < stripes; ++s, q += 32)
      acc = xxh64_round(acc, (uint64_t)load_u32_any(q) | ((uint64_t)load_u32_any(q + 4) << 32));
    uint64_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = (uint64_t)read_lane((uint32_t)acc, k) | ((uint64_t)read_lane((uint32_t)(acc >> 32), k) << 32);
    h = xxh64_converge(v[0], v[1], v[2], v[3]);
  }
  return xxh64_finish(h, UBytes{out}, stripes << 5, n);
}

// -> true and the decoded size, or false.  WRITE_OUT = false decodes without an output (the size query).
template <bool WRITE_OUT>
__device__ __forceinline__ bool decode_chunk(
    const uint8_t* comp_generic, uint64_t n, uint8_t* out_generic, uint64_t cap, uint8_t* lit_generic, uint64_t lit_cap,
    WaveLds& lds, int lane, uint64_t& produced)
{
  cgptr comp = to_global(comp_generic);
  gptr out = to_global(out_generic);
  gptr lit = to_global(lit_generic);
  uint64_t at = 0, outpos = 0;
  while (at < n) {
    const FrameHeader fh = parse_frame_header(UBytes{comp + at}, n - at);
    if (fh.kind == kNoFrame)
      return false;
    if (fh.kind == kSkippableFrame) {
      at += fh.skip_bytes;
      continue;
    }
    at += fh.header_bytes;
    const uint64_t frame_start = outpos;
    SeqState st{0, 0, 0, {1, 4, 8}};
    Entropy en{0, 0, 0, 0, false, false};
    for (;;) {
      const BlockHeader bh = parse_block_header(UBytes{comp + at}, n - at);
      if (!bh.ok)
        return false;
      at += 3;
      if (bh.type == kCompressedBlock) {
        if (bh.size >= kBlockMax)
          return false;
        if (!decode_block<WRITE_OUT>(comp + at, bh.size, out, cap, frame_start, outpos, lit, lit_cap, lds, en, st, lane))
          return false;
      } else {
        if (bh.size > cap - outpos)
          return false;
        if (WRITE_OUT) {
          if (bh.type == kRawBlock) {
            if (bh.size >= 1024u) {
              wave_copy(out + outpos, comp + at, bh.size, lane);
            } else {
              for (uint32_t i = (uint32_t)lane; i < bh.size; i += kWave)
                out[outpos + i] = comp[at + i];
            }
          } else {
            const uint8_t v = UBytes{comp}[at];
            for (uint32_t i = (uint32_t)lane; i < bh.size; i += kWave)
              out[outpos + i] = v;
          }
        }
        outpos += bh.size;
      }
      at += bh.comp_bytes;
      if (bh.last)
        break;
    }
    if (fh.has_size && outpos - frame_start != fh.content_size)
      return false;
    if (fh.checksum) {
      if (n - at < 4)
        return false;
      if (WRITE_OUT) {
        // the wave reads back what its lanes stored
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint64_t h = xxh64_wave(static_cast<cgptr>(out) + frame_start, outpos - frame_start, lane);
        if ((uint32_t)h != (uint32_t)read_le(UBytes{comp + at}, 0, 4))
          return false;
      }
      at += 4;
    }
  }
  produced = outpos;
  return true;
}

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
    const bool ok = decode_chunk<true>(comp, comp_len, out, cap, lit, lit_cap, lds, lane, produced);
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
      good = decode_chunk<false>(comp_generic, n, nullptr, ~(uint64_t)0, nullptr, ~(uint64_t)0, lds, lane, produced);
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
