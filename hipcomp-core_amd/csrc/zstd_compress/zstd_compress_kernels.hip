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
#include <hip/hip_runtime.h>

#include "zstd_codes.hpp"
#include "zstd_compress_launch.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace {

using namespace zstd;

constexpr uint32_t kHashBits = 12;
constexpr uint32_t kHashEntries = 1u << kHashBits;
constexpr uint32_t kStageWords = 256; // 1023 bits left over + 64 x 74 of a trip + a 48-bit field's overhang
constexpr uint32_t kFlushBits = 1024;

// what takes the hash table's place once the parse is over
struct AfterParse
{
  deflate::HuffWork work;
  HufRanks ranks;
  WeightScratch wscratch;
  uint32_t stage[kStageWords];
  FseSym symtt[3][56];
  uint16_t states[3][kMaxTableStates];
};
constexpr uint32_t kScratchBytes = sizeof(AfterParse) > kHashEntries * 2 ? (sizeof(AfterParse) + 15u) / 16u * 16u : kHashEntries * 2;

enum Info { kDescBytes, kLitType, kLitStreams, kLitHeaderBytes, kLitSectionBytes, kSeqHeadBytes, kLogLL, kLogOF, kLogML, kHufUsed, kInfoCount };

struct EncLds
{
  alignas(16) uint8_t scratch[kScratchBytes];
  uint32_t lit_freq[256]; // histogram; from the tree on: code | length << 16 per symbol
  uint32_t code_hist[3][64];
  uint8_t lens[256];
  uint8_t weights[256];
  uint8_t desc[132];
  uint8_t head[32];
  uint8_t seq_head[256];
  uint32_t info[kInfoCount];
  uint32_t stream_bits[4];
};
static_assert(sizeof(EncLds) <= kEncLdsPerWave, "the per-wave LDS budget of zstd_compress_sizing.hpp");

struct GBytes
{
  cgptr p;
  __device__ __forceinline__ uint8_t operator[](uint64_t i) const { return p[i]; }
};

__device__ __forceinline__ uint32_t hash_of(uint32_t v) { return (v * 0x9E3779B1u) >> (32 - kHashBits); }

// the wave reads back what its lanes stored to global memory
__device__ __forceinline__ void global_phase()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- the bit stage ---------------------------------------------------------------------------------------------
// Bits appended lowest first.  Nothing is stored at or beyond dst + limit: a stream that would pass it is
// dropped (ok == false) and the caller writes the chunk another way.
struct BitOut
{
  uint32_t* stage; // LDS, kStageWords, zero beyond `bitpos`
  gptr dst;
  uint32_t bytes;  // stored at dst so far
  uint32_t bitpos; // bits in the stage
  uint32_t limit;
  bool ok;

  __device__ __forceinline__ void init(uint32_t* s, gptr d, uint32_t limit_bytes, int lane)
  {
    stage = s;
    dst = d;
    bytes = 0;
    bitpos = 0;
    limit = limit_bytes;
    ok = true;
    lds_phase();
    for (uint32_t i = (uint32_t)lane; i < kStageWords; i += kWave)
      stage[i] = 0;
    lds_phase();
  }

  // whole dwords out; the started dword moves to the front
  __device__ __forceinline__ void flush_words(int lane)
  {
    const uint32_t words = bitpos >> 5; // < kStageWords - 2
    lds_phase();
    const uint32_t started = stage[words];
    uint32_t mine[kStageWords / kWave];
#pragma unroll
    for (uint32_t j = 0; j < kStageWords / kWave; ++j)
      mine[j] = stage[(uint32_t)lane + kWave * j];
    lds_phase();
    ok = ok && bytes + 4u * words <= limit;
#pragma unroll
    for (uint32_t j = 0; j < kStageWords / kWave; ++j) {
      const uint32_t i = (uint32_t)lane + kWave * j;
      if (ok && i < words)
        store_u32_any(dst + bytes + 4u * i, mine[j]);
      stage[i] = i == 0u ? started : 0u;
    }
    lds_phase();
    bytes += 4u * words;
    bitpos &= 31u;
  }

  __device__ __forceinline__ void or_bits(uint32_t off, uint64_t bits, uint32_t n) // n <= 48
  {
    if (n != 0u) {
      const uint32_t w = off >> 5, s = off & 31u;
      const uint64_t lo = bits << s;
      const uint32_t over = s != 0u ? (uint32_t)(bits >> (64u - s)) : 0u;
      atomicOr(&stage[w], (uint32_t)lo);
      if ((uint32_t)(lo >> 32) != 0u)
        atomicOr(&stage[w + 1u], (uint32_t)(lo >> 32));
      if (over != 0u)
        atomicOr(&stage[w + 2u], over);
    }
  }

  // every lane two fields of at most 48 bits each (a then b), in lane order
  __device__ __forceinline__ void place(uint64_t a, uint32_t na, uint64_t b, uint32_t nb, int lane)
  {
    const uint32_t n = na + nb;
    const uint32_t incl = wave_scan_add_u32(n);
    const uint32_t off = bitpos + incl - n;
    or_bits(off, a, na);
    or_bits(off + na, b, nb);
    bitpos += read_lane(incl, 63);
    if (bitpos >= kFlushBits)
      flush_words(lane);
  }

  // the same bits from all lanes: placed once (n <= 16)
  __device__ __forceinline__ void put(uint32_t bits, uint32_t n, int lane)
  {
    if (lane == 0)
      or_bits(bitpos, bits, n);
    bitpos += n;
    if (bitpos >= kFlushBits)
      flush_words(lane);
  }

  // -> the stream's size in bytes
  __device__ __forceinline__ uint32_t finish(int lane)
  {
    flush_words(lane);
    const uint32_t tail = (bitpos + 7u) >> 3; // <= 4
    lds_phase();
    const uint32_t last = stage[0];
    ok = ok && bytes + tail <= limit;
    if (ok && (uint32_t)lane < tail)
      dst[bytes + (uint32_t)lane] = (uint8_t)(last >> (8u * (uint32_t)lane));
    return bytes + tail;
  }
};

// XXH64, seed 0, of p[0, n): lanes 0-3 hold one accumulator each (the other lanes repeat them), as the decoder does
__device__ __forceinline__ uint64_t xxh64_wave(cgptr p, uint64_t n, int lane)
{
  uint64_t h = kXxhP5;
  const uint64_t stripes = n >> 5;
  if (stripes) {
    const uint32_t j = (uint32_t)lane & 3u;
    uint64_t acc = xxh64_acc_init(j, 0);
    cgptr q = p + 8u * j;
    for (uint64_t s = 0; s < stripes; ++s, q += 32)
      acc = xxh64_round(acc, (uint64_t)load_u32_any(q) | ((uint64_t)load_u32_any(q + 4) << 32));
    uint64_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = (uint64_t)read_lane((uint32_t)acc, k) | ((uint64_t)read_lane((uint32_t)(acc >> 32), k) << 32);
    h = xxh64_converge(v[0], v[1], v[2], v[3]);
  }
  return xxh64_finish(h, GBytes{p}, stripes << 5, n);
}

// frame header, block header, then the caller's payload at the returned offset
__device__ __forceinline__ uint32_t write_heads(gptr dst, uint32_t n, bool checksum, uint32_t type, uint32_t size, EncLds& lds, int lane)
{
  lds_phase();
  if (lane == 0) {
    const uint32_t at = write_frame_header(n, checksum, ByteSink<uint8_t*>{lds.head}, 0u);
    write_block_header(type, size, ByteSink<uint8_t*>{lds.head}, at);
  }
  lds_phase();
  const uint32_t hb = frame_header_bytes(n) + 3u;
  if ((uint32_t)lane < hb)
    dst[lane] = lds.head[lane];
  return hb;
}

// ---- one chunk -------------------------------------------------------------------------------------------------
// src[0, len), len <= 65536 -> dst, -> the frame's size.  rec_a, rec_b: the wave's record buffers, lits: its literal
// buffer (zstd_compress_sizing.hpp).
__device__ __forceinline__ uint32_t zstd_chunk(
    cgptr __restrict__ src, const uint32_t len, gptr __restrict__ dst, uint32_t* rec_a_generic, uint32_t* rec_b_generic,
    uint8_t* lits_generic, const bool checksum, EncLds& lds, const int lane)
{
  HC_GLOBAL uint32_t* rec_a = (HC_GLOBAL uint32_t*)rec_a_generic;
  HC_GLOBAL uint32_t* rec_b = (HC_GLOBAL uint32_t*)rec_b_generic;
  gptr lits = (gptr)lits_generic;
  uint16_t* hash_tab = reinterpret_cast<uint16_t*>(lds.scratch);
  AfterParse& ap = *reinterpret_cast<AfterParse*>(lds.scratch);

  uint32_t block_type = kRawBlock, block_bytes = len;

  // ---- all bytes equal?
  bool all_equal = len >= 2u;
  if (all_equal) {
    const uint32_t first = src[0];
    for (uint32_t i0 = 0; i0 < len; i0 += kWave) {
      const uint32_t i = i0 + (uint32_t)lane;
      if (wave_ballot(i < len && src[i] != first) != 0) {
        all_equal = false;
        break;
      }
    }
  }
  if (all_equal) {
    block_type = kRleBlock;
  } else if (len > 3u) {
    // ---- clear
    {
      const u32x4 z = {0, 0, 0, 0};
      u32x4* p = reinterpret_cast<u32x4*>(lds.scratch);
      for (uint32_t i = (uint32_t)lane; i < kHashEntries * 2 / 16; i += kWave)
        p[i] = z;
      for (uint32_t i = (uint32_t)lane; i < 256u; i += kWave)
        lds.lit_freq[i] = 0;
      for (uint32_t i = (uint32_t)lane; i < 3u * 64u; i += kWave)
        (&lds.code_hist[0][0])[i] = 0;
    }
    lds_phase();

    // ---- parse
    uint32_t nseq = 0, nlit = 0, reg_a = 0, reg_b = 0;
    {
      const uint32_t last_word = len - 4u; // highest readable dword start
      uint32_t pos = 0, pend = 0;
      while (pos < len) {
        const uint32_t my = pos + (uint32_t)lane;
        const uint32_t at = min(my, last_word), over = my - at;
        const uint32_t raw = load_u32_any(src + at);
        const uint32_t data32 = over < 4u ? raw >> (8u * over) : 0u; // (the last three bytes: only their own byte counts)
        const bool valid4 = my <= last_word;
        const uint32_t hash = valid4 ? hash_of(data32) : 0u;
        const uint32_t cand = hash_tab[hash];
        // (an empty slot holds position 0: a candidate like any other, the compare decides)
        const bool probe = valid4 && cand < my;
        const uint32_t theirs = load_u32_any(src + (probe ? cand : 0u));
        const bool hit = probe && theirs == data32;
        const uint64_t hits = wave_ballot(hit);
        const uint32_t in_window = min(len - pos, (uint32_t)kWave);
        const uint32_t t = hits != 0 ? (uint32_t)__builtin_ctzll(hits) : in_window; // literals of this trip
        lds_phase();
        if (valid4 && (uint32_t)lane <= t)
          // Lanes with one slot write it in one ds_write: which of them stays is the hardware's rule (the Deflate
          // encoder's comment on this line).  Any of them is a position of this chunk that the compare validates.
          hash_tab[hash] = (uint16_t)my;
        lds_phase();
        if ((uint32_t)lane < t) {
          atomicAdd(&lds.lit_freq[data32 & 0xFFu], 1u);
          lits[nlit + (uint32_t)lane] = (uint8_t)data32;
        }
        nlit += t;
        if (hits != 0) {
          const uint32_t dist = read_lane(my - cand, (int)t);
          const uint32_t mp = pos + t;
          const uint32_t limit = len - mp;
          uint32_t mlen = kEncMinMatch;
          for (uint32_t j0 = kEncMinMatch; j0 < limit; j0 += kWave) {
            const uint32_t j = j0 + (uint32_t)lane;
            bool differs = true;
            if (j < limit)
              differs = src[mp + j] != src[mp + j - dist];
            const uint64_t d = wave_ballot(differs);
            if (d != 0) {
              mlen = j0 + (uint32_t)__builtin_ctzll(d);
              break;
            }
            mlen = j0 + kWave; // (only where all 64 are below the limit)
          }
          const uint32_t run = pend + t; // < 65536: a match of 4 bytes follows it
          const bool mine = (uint32_t)lane == (nseq & 63u);
          reg_a = mine ? run | (dist << 16) : reg_a;
          reg_b = mine ? mlen : reg_b;
          ++nseq;
          if ((nseq & 63u) == 0u) {
            rec_a[nseq - 64u + (uint32_t)lane] = reg_a;
            rec_b[nseq - 64u + (uint32_t)lane] = reg_b;
          }
          pend = 0;
          pos = mp + mlen;
        } else {
          pend += t;
          pos += t;
        }
      }
      if ((uint32_t)lane < (nseq & 63u)) {
        rec_a[(nseq & ~63u) + (uint32_t)lane] = reg_a;
        rec_b[(nseq & ~63u) + (uint32_t)lane] = reg_b;
      }
    }
    lds_phase();
    global_phase();

    // ---- the codes' histograms: a sequence's offset code needs the offset of the sequence before it, no more
    for (uint32_t i0 = 0; i0 < nseq; i0 += kWave) {
      const uint32_t i = i0 + (uint32_t)lane;
      if (i < nseq) {
        const uint32_t a = rec_a[i], ml = rec_b[i], prev = i ? rec_a[i - 1u] >> 16 : 0u;
        atomicAdd(&lds.code_hist[kLLTable][ll_code(a & 0xFFFFu)], 1u);
        atomicAdd(&lds.code_hist[kOFTable][of_code(offset_value(a >> 16, prev, a & 0xFFFFu))], 1u);
        atomicAdd(&lds.code_hist[kMLTable][ml_code(ml)], 1u);
      }
    }
    lds_phase();

    // ---- the literals' tree.  From here on the hash table's bytes are the work area.
    {
      for (int i = lane; i < 256; i += kWave)
        if (lds.lit_freq[i] != 0u)
          ap.work.order[deflate::rank_of(lds.lit_freq, 256, i)] = (uint16_t)i;
      uint32_t used = 0;
      for (int base = 0; base < 256; base += kWave)
        used += (uint32_t)__builtin_popcountll(wave_ballot(lds.lit_freq[base + lane] != 0u));
      lds_phase();
      if (lane == 0) {
        uint32_t desc_bytes = 0;
        if (used >= 2u) {
          deflate::lengths_from_sorted(lds.lit_freq, 256, (int)used, (int)kHufLogMax, ap.work, lds.lens);
          const uint32_t ll = huf_weights_of(lds.lens, lds.weights);
          huf_codes_of(lds.weights, ll >> 16, lds.lit_freq, ap.ranks);
          desc_bytes = write_weights(lds.weights, ll & 0xFFFFu, ap.wscratch, ByteSink<uint8_t*>{lds.desc}, 0u);
        }
        lds.info[kDescBytes] = desc_bytes;
        lds.info[kHufUsed] = used;
      }
      lds_phase();
    }
    const uint32_t desc_bytes = uniform(lds.info[kDescBytes]), used = uniform(lds.info[kHufUsed]);
    const uint32_t seg = (nlit + 3u) / 4u;
    if (desc_bytes != 0u) {
      // the exact bits of the four quarters
      for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t from = min(k * seg, nlit), to = k == 3u ? nlit : min((k + 1u) * seg, nlit);
        uint32_t bits = 0;
        for (uint32_t i = from + (uint32_t)lane; i < to; i += kWave)
          bits += lds.lit_freq[lits[i]] >> 16;
        bits = read_lane(wave_scan_add_u32(bits), 63);
        if (lane == 0)
          lds.stream_bits[k] = bits;
      }
    }
    lds_phase();

    // ---- the sections' forms
    if (lane == 0) {
      uint32_t sb[4] = {0, 0, 0, 0};
      if (desc_bytes != 0u) {
        sb[0] = lds.stream_bits[0];
        sb[1] = lds.stream_bits[1];
        sb[2] = lds.stream_bits[2];
        sb[3] = lds.stream_bits[3];
      }
      const LiteralsPlan lp = choose_literals(nlit, used == 1u, desc_bytes, sb);
      lds.info[kLitType] = lp.type;
      lds.info[kLitStreams] = lp.streams;
      lds.info[kLitHeaderBytes] = lp.header_bytes;
      lds.info[kLitSectionBytes] = lp.section_bytes;
      write_literals_header(lp, nlit, ByteSink<uint8_t*>{lds.head}, 16u);
      ByteSink<uint8_t*> hs{lds.seq_head};
      if (nseq == 0u) {
        hs(0u, 0);
        lds.info[kSeqHeadBytes] = 1;
      } else {
        uint32_t h = write_seq_count(nseq, hs, 0u);
        const uint32_t modes_at = h++;
        uint32_t modes = 0;
        for (uint32_t t = 0; t < 3u; ++t) {
          const TablePlan tp = plan_table(t, lds.code_hist[t], nseq, ap.symtt[t], ap.states[t], ap.wscratch.fse, hs, h);
          h += tp.head_bytes;
          modes |= tp.mode << (6u - 2u * t);
          lds.info[kLogLL + t] = tp.log;
        }
        hs(modes_at, (uint8_t)modes);
        lds.info[kSeqHeadBytes] = h;
      }
    }
    lds_phase();
    const uint32_t lit_type = uniform(lds.info[kLitType]), lit_streams = uniform(lds.info[kLitStreams]);
    const uint32_t lit_hb = uniform(lds.info[kLitHeaderBytes]), lit_section = uniform(lds.info[kLitSectionBytes]);
    const uint32_t seq_head = uniform(lds.info[kSeqHeadBytes]);
    const uint32_t base = frame_header_bytes(len) + 3u;

    // (a sequences section has at least one byte of bitstream behind its header)
    if (lit_section + seq_head + (nseq ? 1u : 0u) < len) {
      // ---- literals
      gptr block = dst + base;
      bool ok = true;
      if ((uint32_t)lane < lit_hb)
        block[lane] = lds.head[16 + lane];
      if (lit_type == (uint32_t)kRawLit) {
        wave_copy(block + lit_hb, lits, nlit, lane);
      } else if (lit_type == (uint32_t)kRleLit) {
        if (lane == 0)
          block[lit_hb] = lits[0];
      } else {
        for (uint32_t i = (uint32_t)lane; i < desc_bytes; i += kWave)
          block[lit_hb + i] = lds.desc[i];
        uint32_t at = lit_hb + desc_bytes;
        const uint32_t jump = at;
        if (lit_streams == 4u)
          at += 6u;
        BitOut out;
        for (uint32_t k = 0; k < lit_streams; ++k) {
          const uint32_t from = lit_streams == 1u ? 0u : min(k * seg, nlit);
          const uint32_t to = lit_streams == 1u || k == 3u ? nlit : min((k + 1u) * seg, nlit);
          const uint32_t bits = lit_streams == 1u ? lds.stream_bits[0] + lds.stream_bits[1] + lds.stream_bits[2] + lds.stream_bits[3]
                                                  : lds.stream_bits[k];
          const uint32_t size = huf_stream_bytes(uniform(bits));
          out.init(ap.stage, block + at, size, lane);
          for (uint32_t end = to; end > from;) {
            const uint32_t cnt = min(end - from, (uint32_t)kWave);
            uint32_t e = 0;
            if ((uint32_t)lane < cnt)
              e = lds.lit_freq[lits[end - 1u - (uint32_t)lane]];
            out.place(e & 0xFFFFu, e >> 16, 0, 0, lane);
            end -= cnt;
          }
          out.put(1u, 1u, lane);
          ok = out.finish(lane) == size && out.ok && ok; // (the size was summed before: it holds)
          if (lit_streams == 4u && k < 3u && lane < 2)
            block[jump + 2u * k + (uint32_t)lane] = (uint8_t)(size >> (8u * (uint32_t)lane));
          at += size;
        }
      }

      // ---- sequences
      for (uint32_t i = (uint32_t)lane; i < seq_head; i += kWave)
        block[lit_section + i] = lds.seq_head[i];
      uint32_t stream_bytes = 0;
      if (nseq != 0u) {
        const uint32_t log_ll = uniform(lds.info[kLogLL]), log_of = uniform(lds.info[kLogOF]), log_ml = uniform(lds.info[kLogML]);
        const uint32_t t = (uint32_t)lane < 3u ? (uint32_t)lane : 2u; // lane 0: LL, lane 1: OF, lanes 2 ..: ML
        const FseSym* symtt = ap.symtt[t];
        const uint16_t* states = ap.states[t];
        uint32_t state = 0;
        BitOut out;
        // the block stays below len bytes
        out.init(ap.stage, block + lit_section + seq_head, len - 1u - lit_section - seq_head, lane);
        for (uint32_t s0 = 0; s0 < nseq; s0 += kWave) {
          const uint32_t cnt = min(nseq - s0, (uint32_t)kWave);
          // lane j: sequence nseq - 1 - (s0 + j)
          uint32_t ll = 0, ml = 3, ov = 4, packed = 0;
          if ((uint32_t)lane < cnt) {
            const uint32_t i = nseq - 1u - s0 - (uint32_t)lane;
            const uint32_t a = rec_a[i], prev = i ? rec_a[i - 1u] >> 16 : 0u;
            ml = rec_b[i];
            ll = a & 0xFFFFu;
            ov = offset_value(a >> 16, prev, ll);
            packed = ll_code(ll) | (of_code(ov) << 8) | (ml_code(ml) << 16);
          }
          uint32_t e_ll = 0, e_of = 0, e_ml = 0;
          for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t code = (read_lane(packed, (int)k) >> (8u * t)) & 0xFFu;
            uint32_t e = 0;
            if (s0 == 0u && k == 0u)
              state = fse_init(symtt, states, code);
            else
              e = fse_encode(symtt, states, state, code);
            const uint32_t r0 = read_lane(e, 0), r1 = read_lane(e, 1), r2 = read_lane(e, 2);
            if ((uint32_t)lane == k) {
              e_ll = r0;
              e_of = r1;
              e_ml = r2;
            }
          }
          // OF, ML, LL state bits, then the LL, ML, OF extra bits
          const uint32_t llc = packed & 0xFFu, ofc = (packed >> 8) & 0xFFu, mlc = packed >> 16;
          const uint32_t n_of = e_of >> 16, n_ml = e_ml >> 16, n_ll = e_ll >> 16;
          uint64_t a = (uint64_t)(e_of & 0xFFFFu) | ((uint64_t)(e_ml & 0xFFFFu) << n_of) | ((uint64_t)(e_ll & 0xFFFFu) << (n_of + n_ml));
          uint32_t na = n_of + n_ml + n_ll;
          uint64_t b = 0;
          uint32_t nb = 0;
          if ((uint32_t)lane < cnt) {
            a |= (uint64_t)(ll - kLLBase[llc]) << na;
            na += kLLBits[llc];
            b = (uint64_t)(ml - kMLBase[mlc]) | ((uint64_t)(ov - (1u << ofc)) << kMLBits[mlc]);
            nb = kMLBits[mlc] + ofc;
          } else {
            na = 0;
          }
          out.place(a, na, b, nb, lane);
        }
        const uint32_t s_ll = read_lane(state, 0), s_of = read_lane(state, 1), s_ml = read_lane(state, 2);
        out.put(s_ml & ((1u << log_ml) - 1u), log_ml, lane);
        out.put(s_of & ((1u << log_of) - 1u), log_of, lane);
        out.put(s_ll & ((1u << log_ll) - 1u), log_ll, lane);
        out.put(1u, 1u, lane);
        stream_bytes = out.finish(lane);
        ok = ok && out.ok;
      }
      if (ok) {
        block_type = kCompressedBlock;
        block_bytes = lit_section + seq_head + stream_bytes;
      }
    }
  }

  // ---- frame
  const uint32_t base = write_heads(dst, len, checksum, block_type, block_type == (uint32_t)kCompressedBlock ? block_bytes : len, lds, lane);
  uint32_t at = base;
  if (block_type == (uint32_t)kRleBlock) {
    if (lane == 0)
      dst[at] = src[0];
    at += 1u;
  } else if (block_type == (uint32_t)kRawBlock) {
    wave_copy(dst + at, src, len, lane);
    at += len;
  } else {
    at += block_bytes;
  }
  if (checksum) {
    const uint32_t h = (uint32_t)xxh64_wave(src, len, lane);
    if (lane < 4)
      dst[at + (uint32_t)lane] = (uint8_t)(h >> (8u * (uint32_t)lane));
    at += 4u;
  }
  return at;
}

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
    const uint32_t c = size <= (size_t)max_chunk ? zstd_chunk(src, (uint32_t)size, dst, rec_a, rec_b, lits, checksum != 0u, lds, lane) : 0u;
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
