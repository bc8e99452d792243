// deflate_compress_kernels.hip -- batched raw-Deflate (RFC 1951) encoder for gfx950, one chunk per wavefront.
//
// Shape:
//   * One wave per workgroup with its own LDS; chunks are taken grid-stride, so the grid -- and with it the temp
//     space, one token buffer per wave -- is bounded whatever the batch.  Waves share nothing and never wait for
//     one another.
//   * Parse: greedy LZ77, 64 positions per trip.  Every lane hashes the 4 bytes at its position, looks its slot
//     of a 4096-entry table of 16-bit positions up, validates the candidate by comparing the 4 bytes, a ballot
//     picks the first hit; the match is extended 64 bytes per step to at most 258.  The lanes up to the hit
//     post their positions.  Tokens leave as 32-bit records {literal run, match length, distance} to the wave's
//     buffer in temp space, 64 records per store; the histograms are counted in LDS as the parse goes.
//   * Codes: deflate_codes.hpp.  The sort of the symbols runs over the lanes (rank_of), the rest -- a few hundred
//     steps -- on one lane.
//   * Choice: exact cost of the tokens as one dynamic block, one fixed block and as stored blocks; the smallest
//     is written, so no stream is longer than the stored form.
//   * Emit: per trip up to 64 literals and the match behind them; a prefix sum of the bit lengths places every
//     lane's code with ds_or_b32 into a zeroed LDS stage, whole dwords of which leave with one store per lane.
//   * Bounds: a chunk reads [src, src + len) and its own token buffer, and writes at most stored_bytes(len).
#include <hip/hip_runtime.h>

#include "deflate_codes.hpp"
#include "deflate_compress_launch.hpp"
#include "wave_utils.hpp"

namespace hcamd {
namespace {

using namespace deflate;

constexpr uint32_t kHashBits = 12;
constexpr uint32_t kHashEntries = 1u << kHashBits;
constexpr uint32_t kMaxLitRun = 255;     // per record
constexpr uint32_t kStageWords = 68;     // 1023 bits left over + 993 of a trip + a 48-bit code's overhang
constexpr uint32_t kFlushBits = 1024;

// The hash table is dead once the parse is over: the code builder's work arrays, the code-length stream and the
// bit stage take its place.
constexpr uint32_t kScratchBytes = kHashEntries * 2;
constexpr uint32_t kClSymsAt = 4096, kStageAt = 4096 + 2 * 320;
static_assert(sizeof(HuffWork) <= kClSymsAt && kStageAt + 4 * kStageWords <= kScratchBytes, "the scratch area's layout");

struct EncLds
{
  alignas(16) uint8_t scratch[kScratchBytes];
  uint32_t lit_freq[kFixedLitLen];  // histogram; from the choice on: code | length << 16 per symbol
  uint32_t dist_freq[kFixedDist];
  uint8_t lit_lens[kFixedLitLen];
  uint8_t dist_lens[kFixedDist];
  uint16_t lit_codes[kFixedLitLen];
  uint16_t dist_codes[kFixedDist];
  uint32_t cl_freq[kNumCodeLen + 1];
  uint16_t cl_codes[kNumCodeLen + 1];
  uint8_t cl_lens[kNumCodeLen + 1];
  uint32_t info[5]; // lane 0's results: HLIT, HDIST, HCLEN, symbols of the code-length stream, block kind
};
static_assert(sizeof(EncLds) <= 12 * 1024, "the per-wave LDS budget of DESIGN.md section 14");

__device__ __forceinline__ uint32_t hash_of(uint32_t v) { return (v * 0x9E3779B1u) >> (32 - kHashBits); }

// ---- the bit stage ---------------------------------------------------------------------------------------------
struct BitOut
{
  uint32_t* stage; // LDS, kStageWords, zero beyond `bitpos`
  gptr dst;
  uint32_t bytes;  // stored at dst so far
  uint32_t bitpos; // bits in the stage

  __device__ __forceinline__ void init(uint32_t* s, gptr d, int lane)
  {
    stage = s;
    dst = d;
    bytes = 0;
    bitpos = 0;
    lds_phase();
    for (uint32_t i = (uint32_t)lane; i < kStageWords; i += kWave)
      stage[i] = 0;
    lds_phase();
  }

  // whole dwords out, one per lane; the started dword moves to the front
  __device__ __forceinline__ void flush_words(int lane)
  {
    const uint32_t words = bitpos >> 5; // < 64
    lds_phase();
    const uint32_t mine = stage[lane];
    const uint32_t started = stage[words];
    lds_phase();
    if ((uint32_t)lane < words)
      store_u32_any(dst + bytes + 4u * (uint32_t)lane, mine);
    for (uint32_t i = (uint32_t)lane; i < kStageWords; i += kWave)
      stage[i] = i == 0u ? started : 0u;
    lds_phase();
    bytes += 4u * words;
    bitpos &= 31u;
  }

  // every lane its own code of n <= 48 bits (n == 0: none), in lane order
  __device__ __forceinline__ void place(uint64_t bits, uint32_t n, int lane)
  {
    const uint32_t incl = wave_scan_add_u32(n);
    const uint32_t off = bitpos + incl - n;
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
    bitpos += read_lane(incl, 63);
    if (bitpos >= kFlushBits)
      flush_words(lane);
  }

  // the same bits from all lanes: placed once (n <= 16)
  __device__ __forceinline__ void put(uint32_t bits, uint32_t n, int lane)
  {
    if (lane == 0 && n != 0u) {
      const uint32_t w = bitpos >> 5, s = bitpos & 31u;
      const uint64_t lo = (uint64_t)bits << s;
      atomicOr(&stage[w], (uint32_t)lo);
      if ((uint32_t)(lo >> 32) != 0u)
        atomicOr(&stage[w + 1u], (uint32_t)(lo >> 32));
    }
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
    if ((uint32_t)lane < tail)
      dst[bytes + (uint32_t)lane] = (uint8_t)(last >> (8u * (uint32_t)lane));
    return bytes + tail;
  }
};

// ---- stored blocks ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t write_stored(cgptr __restrict__ src, uint32_t len, gptr __restrict__ dst, int lane)
{
  uint32_t at = 0, from = 0, left = len;
  do {
    const uint32_t n = left < kStoredBlockMax ? left : kStoredBlockMax;
    const uint32_t final_block = left == n ? 1u : 0u;
    const uint32_t word = n | ((n ^ 0xFFFFu) << 16);
    if (lane < 5)
      dst[at + (uint32_t)lane] = (uint8_t)(lane == 0 ? final_block : word >> (8u * (uint32_t)(lane - 1)));
    wave_copy(dst + at + 5u, src + from, n, lane);
    at += 5u + n;
    from += n;
    left -= n;
  } while (left != 0u);
  return at;
}

// ---- one chunk -------------------------------------------------------------------------------------------------
// src[0, len), len <= 65536 -> dst, -> the stream's size.  tokens: the wave's record buffer (len / 4 + 2 records,
// rounded up to 64).
__device__ __forceinline__ uint32_t deflate_chunk(
    cgptr __restrict__ src, const uint32_t len, gptr __restrict__ dst, uint32_t* __restrict__ tokens_generic, EncLds& lds,
    const int lane)
{
  HC_GLOBAL uint32_t* tokens = (HC_GLOBAL uint32_t*)tokens_generic;
  uint16_t* hash_tab = reinterpret_cast<uint16_t*>(lds.scratch);
  // ---- clear
  {
    const u32x4 z = {0, 0, 0, 0};
    u32x4* p = reinterpret_cast<u32x4*>(lds.scratch);
    for (uint32_t i = (uint32_t)lane; i < kScratchBytes / 16; i += kWave)
      p[i] = z;
    for (uint32_t i = (uint32_t)lane; i < (uint32_t)kFixedLitLen; i += kWave)
      lds.lit_freq[i] = 0;
    if (lane < kFixedDist)
      lds.dist_freq[lane] = 0;
    // (the code builder fills 286 + 30 + 19 lengths; the codes are assigned over 288 + 32 + 19)
    for (uint32_t i = (uint32_t)lane; i < (uint32_t)kFixedLitLen; i += kWave)
      lds.lit_lens[i] = 0;
    if (lane < kFixedDist)
      lds.dist_lens[lane] = 0;
    if (lane <= kNumCodeLen)
      lds.cl_lens[lane] = 0;
  }
  lds_phase();

  // ---- parse
  uint32_t nrec = 0, rec_reg = 0;
  auto push = [&](uint32_t rec) {
    rec_reg = (uint32_t)lane == (nrec & 63u) ? rec : rec_reg;
    ++nrec;
    if ((nrec & 63u) == 0u)
      tokens[nrec - 64u + (uint32_t)lane] = rec_reg;
  };
  {
    const uint32_t last_word = len >= 4u ? len - 4u : 0u; // highest readable dword start
    uint32_t pos = 0, pend = 0;
    while (pos < len) {
      const uint32_t my = pos + (uint32_t)lane;
      uint32_t data32 = 0, cand = 0;
      bool valid4 = false, hit = false;
      if (len >= 4u) {
        const uint32_t at = min(my, last_word), over = my - at;
        const uint32_t raw = load_u32_any(src + at);
        data32 = over < 4u ? raw >> (8u * over) : 0u; // (the last three bytes: only their own byte counts)
        valid4 = my <= last_word;
      } else if (my < len) {
        data32 = src[my];
      }
      const uint32_t hash = valid4 ? hash_of(data32) : 0u;
      if (len >= 4u) {
        cand = hash_tab[hash];
        // (an empty slot holds position 0: a candidate like any other, the compare decides)
        const bool probe = valid4 && cand < my && my - cand <= kMaxDistance;
        const uint32_t theirs = load_u32_any(src + (probe ? cand : 0u));
        hit = probe && theirs == data32;
      }
      const uint64_t hits = wave_ballot(hit);
      const uint32_t in_window = min(len - pos, (uint32_t)kWave);
      const uint32_t t = hits != 0 ? (uint32_t)__builtin_ctzll(hits) : in_window; // literals of this trip
      lds_phase();
      if (valid4 && (uint32_t)lane <= t)
        // Lanes with one slot write it in one ds_write: which of them stays is the hardware's rule, not the ISA's
        // promise (on gfx950 the highest lane, as the Snappy encoder's straight path finds too).  Any of them is a
        // position of this chunk that the compare validates, so the stream is right whichever stays; the BYTES are
        // the same from run to run and place to place on one device model, which is what the header promises.
        hash_tab[hash] = (uint16_t)my;
      lds_phase();
      if ((uint32_t)lane < t)
        atomicAdd(&lds.lit_freq[data32 & 0xFFu], 1u);
      if (hits != 0) {
        const uint32_t dist = read_lane(my - cand, (int)t);
        const uint32_t mp = pos + t;
        const uint32_t limit = min(kMaxMatch, len - mp);
        uint32_t mlen = kMinMatch;
        for (uint32_t j0 = kMinMatch; j0 < limit; j0 += kWave) {
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
        const uint32_t lit = pend + t; // <= 191 + 63: pend is sent off once it passes kMaxLitRun - kWave
        push((lit << 24) | (mlen << 15) | (dist - 1u));
        pend = 0;
        if (lane == 0) {
          atomicAdd(&lds.lit_freq[length_symbol(mlen)], 1u);
          atomicAdd(&lds.dist_freq[dist_symbol(dist)], 1u);
        }
        pos = mp + mlen;
      } else {
        pend += t;
        if (pend > kMaxLitRun - kWave) {
          push(pend << 24);
          pend = 0;
        }
        pos += t;
      }
    }
    push(pend << 24);
    if ((uint32_t)lane < (nrec & 63u))
      tokens[(nrec & ~63u) + (uint32_t)lane] = rec_reg;
  }
  lds_phase();

  // ---- codes.  From here on the hash table's bytes are the work area.
  HuffWork& work = *reinterpret_cast<HuffWork*>(lds.scratch);
  uint16_t* cl_syms = reinterpret_cast<uint16_t*>(lds.scratch + kClSymsAt);
  uint32_t* stage = reinterpret_cast<uint32_t*>(lds.scratch + kStageAt);
  if (lane == 0)
    lds.lit_freq[kEndOfBlock] = 1;
  lds_phase();
  auto lengths_of = [&](const uint32_t* freq, int n, int maxbits, uint8_t* lens, bool complete) {
    // build_lengths() with its sort spread over the lanes: rank_of() per symbol here, lengths_from_sorted() on one
    for (int i = lane; i < n; i += kWave)
      if (freq[i] != 0u)
        work.order[rank_of(freq, n, i)] = (uint16_t)i;
    uint32_t used = 0;
    for (int base = 0; base < n; base += kWave)
      used += (uint32_t)__builtin_popcountll(wave_ballot(base + lane < n && freq[base + lane] != 0u));
    lds_phase();
    if (lane == 0)
      lengths_from_sorted(freq, n, (int)used, maxbits, work, lens, complete);
    lds_phase();
  };
  lengths_of(lds.lit_freq, kMaxLitLen, kMaxBits, lds.lit_lens, false);
  lengths_of(lds.dist_freq, kMaxDist, kMaxBits, lds.dist_lens, false);
  if (lane == 0) {
    const int hlit = trimmed_hlit(lds.lit_lens), hdist = trimmed_hdist(lds.dist_lens);
    lds.info[0] = (uint32_t)hlit;
    lds.info[1] = (uint32_t)hdist;
    lds.info[3] = (uint32_t)code_length_stream(lds.lit_lens, hlit, lds.dist_lens, hdist, cl_syms, lds.cl_freq);
  }
  lds_phase();
  lengths_of(lds.cl_freq, kNumCodeLen, kCodeLenMaxBits, lds.cl_lens, true);
  if (lane == 0) {
    const int hclen = trimmed_hclen(lds.cl_lens);
    lds.info[2] = (uint32_t)hclen;
    const uint32_t dyn = dynamic_cost(lds.lit_freq, lds.dist_freq, lds.lit_lens, lds.dist_lens, lds.cl_freq, lds.cl_lens, hclen);
    const uint32_t fix = fixed_cost(lds.lit_freq, lds.dist_freq);
    lds.info[4] = (uint32_t)choose_block(stored_cost(len), fix, dyn);
  }
  lds_phase();
  const uint32_t hlit = uniform(lds.info[0]), hdist = uniform(lds.info[1]), hclen = uniform(lds.info[2]);
  const uint32_t ncl = uniform(lds.info[3]), kind = uniform(lds.info[4]);

  // ---- choice
  if (kind == (uint32_t)kStored)
    return write_stored(src, len, dst, lane);
  if (kind == (uint32_t)kFixed) {
    for (uint32_t i = (uint32_t)lane; i < (uint32_t)kFixedLitLen; i += kWave)
      lds.lit_lens[i] = (uint8_t)fixed_litlen_length(i);
    if (lane < kFixedDist)
      lds.dist_lens[lane] = (uint8_t)kFixedDistLength;
    lds_phase();
  }
  if (lane == 0) {
    assign_codes(lds.lit_lens, kFixedLitLen, work, lds.lit_codes);
    assign_codes(lds.dist_lens, kFixedDist, work, lds.dist_codes);
    assign_codes(lds.cl_lens, kNumCodeLen, work, lds.cl_codes);
  }
  lds_phase();
  // code | length << 16 per symbol, where the histograms were
  uint32_t* lit_tab = lds.lit_freq;
  uint32_t* dist_tab = lds.dist_freq;
  for (uint32_t i = (uint32_t)lane; i < (uint32_t)kFixedLitLen; i += kWave)
    lit_tab[i] = (uint32_t)lds.lit_codes[i] | ((uint32_t)lds.lit_lens[i] << 16);
  if (lane < kFixedDist)
    dist_tab[lane] = (uint32_t)lds.dist_codes[lane] | ((uint32_t)lds.dist_lens[lane] << 16);
  lds_phase();

  // ---- emit
  BitOut out;
  out.init(stage, dst, lane);
  if (kind == (uint32_t)kFixed) {
    out.put(1u | (1u << 1), 3u, lane);
  } else {
    put_dynamic_header([&](uint32_t v, uint32_t n) { out.put(v, n, lane); }, (int)hlit, (int)hdist, (int)hclen, lds.cl_lens);
    for (uint32_t base = 0; base < ncl; base += kWave) {
      uint64_t bits = 0;
      uint32_t n = 0;
      if (base + (uint32_t)lane < ncl) {
        const uint32_t e = cl_syms[base + (uint32_t)lane], sym = e & 0xFFu, l = lds.cl_lens[sym];
        bits = (uint64_t)((uint32_t)lds.cl_codes[sym] | ((e >> 8) << l));
        n = l + code_len_extra_bits(sym);
      }
      out.place(bits, n, lane);
    }
  }
  uint32_t ip = 0;
  for (uint32_t r0 = 0; r0 < nrec; r0 += kWave) {
    const uint32_t count = min(nrec - r0, (uint32_t)kWave);
    const uint32_t recs = (uint32_t)lane < count ? tokens[r0 + (uint32_t)lane] : 0u;
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t rec = read_lane(recs, (int)k);
      uint32_t lit = rec >> 24;
      const uint32_t mlen = (rec >> 15) & 511u, dist = (rec & 32767u) + 1u;
      bool match = mlen != 0u;
      uint64_t mbits = 0;
      uint32_t mn = 0;
      if (match) {
        const uint32_t ls = length_symbol(mlen), ds = dist_symbol(dist);
        const uint32_t le = uniform(lit_tab[ls]), de = uniform(dist_tab[ds]);
        const uint32_t ll = le >> 16, lx = length_extra(ls - 257u), dl = de >> 16, dx = dist_extra(ds);
        mbits = (uint64_t)(le & 0xFFFFu) | ((uint64_t)(mlen - length_base(ls - 257u)) << ll)
                | ((uint64_t)(de & 0xFFFFu) << (ll + lx)) | ((uint64_t)(dist - dist_base(ds)) << (ll + lx + dl));
        mn = ll + lx + dl + dx;
      }
      while (lit != 0u || match) {
        const uint32_t n = min(lit, (uint32_t)kWave);
        const bool carries = match && n < (uint32_t)kWave; // the match rides behind the run's last literals
        uint64_t bits = 0;
        uint32_t nb = 0;
        if ((uint32_t)lane < n) {
          const uint32_t e = lit_tab[src[ip + (uint32_t)lane]];
          bits = e & 0xFFFFu;
          nb = e >> 16;
        } else if (carries && (uint32_t)lane == n) {
          bits = mbits;
          nb = mn;
        }
        out.place(bits, nb, lane);
        ip += n;
        lit -= n;
        if (carries) {
          ip += mlen;
          match = false;
        }
      }
    }
  }
  const uint32_t eob = uniform(lit_tab[kEndOfBlock]);
  out.put(eob & 0xFFFFu, eob >> 16, lane);
  return out.finish(lane);
}

__global__ __launch_bounds__(kWave) void deflate_compress_kernel(
    const uint8_t* const* __restrict__ in_ptrs, const size_t* __restrict__ in_bytes, const uint32_t max_chunk,
    const size_t batch, uint32_t* __restrict__ temp, const uint32_t records_per_wave, uint8_t* const* __restrict__ out_ptrs,
    size_t* __restrict__ out_bytes)
{
  __shared__ EncLds lds;
  const int lane = (int)threadIdx.x;
  uint32_t* tokens = temp + (size_t)blockIdx.x * records_per_wave;
  for (size_t chunk = blockIdx.x; chunk < batch; chunk += gridDim.x) {
    cgptr src = to_global(uniform_ptr(in_ptrs[chunk]));
    const size_t size = (size_t)uniform((uint64_t)in_bytes[chunk]);
    gptr dst = to_global(uniform_ptr(out_ptrs[chunk]));
    // (a chunk above the limit the call was given: neither its tokens nor its stream would have room)
    const uint32_t c = size <= (size_t)max_chunk ? deflate_chunk(src, (uint32_t)size, dst, tokens, lds, lane) : 0u;
    if (lane == 0)
      out_bytes[chunk] = c;
    lds_phase();
  }
}

} // namespace

size_t deflate_compress_records_per_wave(size_t max_chunk_bytes)
{
  // a record per match of at least 4 bytes or per literal run, and the last one; stored 64 at a time
  return (max_chunk_bytes / deflate::kMinMatch + 2 + 63) / 64 * 64;
}

size_t deflate_compress_waves(size_t batch)
{
  return batch < kDeflateCompressMaxWaves ? batch : kDeflateCompressMaxWaves;
}

void deflate_launch_compress(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t max_chunk_bytes, size_t batch, void* temp,
    uint8_t* const* out_ptrs, size_t* out_bytes, hipStream_t stream)
{
  deflate_compress_kernel<<<dim3((unsigned)deflate_compress_waves(batch)), dim3(kWave), 0, stream>>>(
      in_ptrs, in_bytes, (uint32_t)max_chunk_bytes, batch, reinterpret_cast<uint32_t*>(temp),
      (uint32_t)deflate_compress_records_per_wave(max_chunk_bytes), out_ptrs, out_bytes);
}

} // namespace hcamd
