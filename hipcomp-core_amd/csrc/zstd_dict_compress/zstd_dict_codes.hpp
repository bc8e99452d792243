// zstd_dict_codes.hpp -- what a dictionary adds to the format logic of the Zstandard encoder, free of HIP.
//
// Constexpr and plain C++17 like ../zstd_compress/zstd_codes.hpp, on which it builds: the kernels
// (zstd_dict_compress_kernels.hip, ../zstd_compress/zstd_encode.hiph) and the CPU driver
// (tests/zstd_dict_codes_driver.cpp) include this one file.  It holds
//
//   hash_of                                   the parse's hash, one copy for the kernels and for prime_table
//   EncBlobHeader, DictTables, kEncBlob...    the layout of the blob that a dictionary is digested into for compression
//   tail_of, prime_table                      what of the content is searched, and the match table it starts from
//   build_dict_tables, prepare_scalar         dictionary -> encoding tables -> blob
//   choose_literals_dict, plan_table_dict     the section forms with one more candidate each: Treeless literals
//                                             under the dictionary's code, Repeat_Mode under its distribution
//   write_frame_header_dict                   the frame header with the Dictionary_ID field
//   encode_frame_dict                         the scalar encoder of a token list against a blob
//
// Rules that the format leaves to an encoder, as this one sets them (the others are zstd_codes.hpp's):
//   * Only the last kDictEncMaxTail bytes of the content are searched, and none where the content is shorter than
//     8 bytes (libzstd ignores such content when it compresses).  History is tail ++ chunk, at most 65536 bytes.
//   * The first sequence's "offset of the sequence before it" is the dictionary's first repeat offset; repeat
//     offsets 2 and 3 stay unused.
//   * Literals: Treeless where every literal has a code in the dictionary's table and the section is no longer than
//     with a tree of its own (a tie goes to Treeless); raw and RLE keep their ties.
//   * Tables: at equal cost predefined, then Repeat_Mode, then described; one used code stays RLE.
#pragma once

#include <cstdint>

#include "zstd_codes.hpp"
#include "zstd_dict.hpp"

namespace hcamd {
namespace zstd {

constexpr uint32_t kEncHashBits = 12;
constexpr uint32_t kEncHashEntries = 1u << kEncHashBits;
constexpr uint32_t hash_of(uint32_t v) { return (v * 0x9E3779B1u) >> (32 - kEncHashBits); }

constexpr uint32_t kDictEncMaxChunk = 32768;
constexpr uint32_t kDictEncMaxTail = 32768;
constexpr uint32_t kDictEncMinContent = 8;
constexpr uint32_t kDictFrameOverhead = 18; // kFrameOverhead + 4 bytes of Dictionary_ID
constexpr uint32_t dict_frame_bound(uint32_t n) { return n + kDictFrameOverhead; }

// ---- the blob ---------------------------------------------------------------------------------------------------------
// header | primed match table, 4096 x uint16 | DictTables | tail, zeros to the blob's end.  No pointers.
constexpr uint32_t kEncBlobMagic = 0x45435A48u; // "HZCE"
constexpr uint32_t kEncBlobVersion = 1;
struct EncBlobHeader
{
  uint32_t magic, version, valid, dict_id, has_entropy;
  uint32_t rep[3];
  uint32_t content_size, tail;
  uint32_t ll_log, of_log, ml_log;
  uint32_t reserved[3];
};
static_assert(sizeof(EncBlobHeader) == 64, "the blob's header is 64 bytes");

// The dictionary's encoding tables as the kernel keeps its own: huf[] as lit_freq after huf_codes_of (code | length <<
// 16), symtt / states as AfterParse's, in the order LL, OF, ML; norm[] is what Repeat_Mode's cost is taken under.
struct DictTables
{
  uint32_t huf[256];
  FseSym symtt[3][56];
  uint16_t states[3][kMaxTableStates];
  int16_t norm[3][64];
};
constexpr uint32_t kEncBlobAlign = 16;
constexpr uint32_t kEncBlobTable = sizeof(EncBlobHeader);
constexpr uint32_t kEncBlobTables = kEncBlobTable + 2u * kEncHashEntries;
constexpr uint32_t kEncBlobTail = kEncBlobTables + (uint32_t)sizeof(DictTables);
static_assert(kEncBlobTail == 14080 && kEncBlobTables % kEncBlobAlign == 0 && kEncBlobTail % kEncBlobAlign == 0,
              "HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES; sections start at 16-byte boundaries");

// a function of dict_bytes alone: whatever the sections take, the tail is no longer than the dictionary
constexpr uint64_t enc_prepared_bytes(uint64_t dict_bytes)
{
  const uint64_t m = dict_bytes < kDictEncMaxTail ? dict_bytes : kDictEncMaxTail;
  return kEncBlobTail + (m + (kEncBlobAlign - 1u)) / kEncBlobAlign * kEncBlobAlign;
}

// T: how many bytes of the content's end are searched
constexpr uint32_t tail_of(uint32_t content_size)
{
  return content_size < kDictEncMinContent ? 0u : content_size < kDictEncMaxTail ? content_size : kDictEncMaxTail;
}

// Slot h: the greatest v in [0, T - 4] whose 4 bytes hash to h, 0 where there is none.  (A definition: the kernel
// reaches it with atomicMax, this loop by going up.)
template <class C, class M>
constexpr void prime_table(C tail, uint32_t t, M& table)
{
  for (uint32_t h = 0; h < kEncHashEntries; ++h)
    table[h] = 0;
  for (uint32_t v = 0; v + 4u <= t; ++v)
    table[hash_of((uint32_t)read_le(tail, v, 4))] = (uint16_t)v;
}

struct DictScratch
{
  uint8_t weights[256];
  int16_t norm[256];
  FseEntry wtable[64];
  uint16_t next[256];
  HufRanks ranks;
  FseScratch fse;
};

template <class P>
constexpr DictLayout dict_verdict(P p, uint32_t n, DictScratch& s)
{
  return parse_dictionary(p, n, s.weights, s.norm, s.wtable, s.next);
}

// the descriptions of a formatted dictionary that passed dict_verdict -> t (all of it: what no table uses is 0),
// logs[] in the order LL, OF, ML
template <class P>
constexpr void build_dict_tables(P p, uint32_t n, const DictLayout& d, DictScratch& s, DictTables& t, uint32_t (&logs)[3])
{
  for (uint32_t i = 0; i < 256u; ++i) {
    s.weights[i] = 0;
    t.huf[i] = 0;
  }
  for (uint32_t k = 0; k < 3u; ++k) {
    for (uint32_t i = 0; i < 56u; ++i)
      t.symtt[k][i] = FseSym{0u, 0};
    for (uint32_t i = 0; i < kMaxTableStates; ++i)
      t.states[k][i] = 0;
  }
  const HufDesc hd = read_huf_weights(p + d.huf_at, n - d.huf_at, s.weights, s.norm, s.wtable, s.next);
  for (uint32_t i = hd.nsym; i < 256u; ++i)
    s.weights[i] = 0;
  huf_codes_of(s.weights, hd.log, t.huf, s.ranks);
  const uint32_t at[3] = {d.ll_at, d.of_at, d.ml_at};
  const uint32_t max_sym[3] = {kLLSymMax, kOFSymMax, kMLSymMax};
  for (uint32_t k = 0; k < 3u; ++k) {
    const NCount nc = read_ncount(p + at[k], n - at[k], s.norm, max_sym[k], kTableMaxLog[k]);
    for (uint32_t i = 0; i < 64u; ++i)
      t.norm[k][i] = (int16_t)(i < nc.nsym ? s.norm[i] : 0);
    fse_build_ctable(t.norm[k], kTableSyms[k], nc.log, t.symtt[k], t.states[k], s.fse.spread, s.fse.cumul);
    logs[k] = nc.log;
  }
}

constexpr EncBlobHeader invalid_blob_header()
{
  return EncBlobHeader{kEncBlobMagic, kEncBlobVersion, 0, 0, 0, {0, 0, 0}, 0, 0, 0, 0, 0, {0, 0, 0}};
}

struct PrepareWork
{
  DictScratch scratch;
  DictTables tables;
  uint16_t table[kEncHashEntries];
};

// dict[0, n), n <= kDictBytesMax -> blob[0, enc_prepared_bytes(n)); -> false where the dictionary is refused, and
// then only the header is written, marked invalid.  (The host's byte order is the device's: little-endian.)
inline bool prepare_scalar(const uint8_t* dict, uint32_t n, PrepareWork& w, uint8_t* blob)
{
  auto put = [&](uint32_t at, const void* from, uint32_t bytes) {
    const uint8_t* f = static_cast<const uint8_t*>(from);
    for (uint32_t i = 0; i < bytes; ++i)
      blob[at + i] = f[i];
  };
  EncBlobHeader h = invalid_blob_header();
  const DictLayout d = dict_verdict(dict, n, w.scratch);
  if (!d.ok) {
    put(0, &h, sizeof h);
    return false;
  }
  const uint32_t size = (uint32_t)enc_prepared_bytes(n);
  for (uint32_t i = 0; i < size; ++i)
    blob[i] = 0;
  h.valid = 1;
  h.dict_id = d.dict_id;
  h.rep[0] = d.rep[0];
  h.rep[1] = d.rep[1];
  h.rep[2] = d.rep[2];
  h.content_size = d.content_size;
  h.tail = tail_of(d.content_size);
  if (d.formatted) {
    uint32_t logs[3] = {0, 0, 0};
    build_dict_tables(dict, n, d, w.scratch, w.tables, logs);
    h.has_entropy = 1;
    h.ll_log = logs[0];
    h.of_log = logs[1];
    h.ml_log = logs[2];
    put(kEncBlobTables, &w.tables, sizeof w.tables);
  }
  const uint8_t* tail = dict + d.content_at + d.content_size - h.tail;
  prime_table(tail, h.tail, w.table);
  put(kEncBlobTable, w.table, sizeof w.table);
  put(kEncBlobTail, tail, h.tail);
  put(0, &h, sizeof h);
  return true;
}

// ---- the section forms -------------------------------------------------------------------------------------------------
// choose_literals with the Treeless candidate: dict_bits[] are stream_bits[] taken with the dictionary's lengths,
// dict_legal says that every literal used has a code there.
constexpr LiteralsPlan choose_literals_dict(uint32_t n, bool all_equal, uint32_t desc_bytes, const uint32_t stream_bits[4],
                                            bool dict_legal, const uint32_t dict_bits[4], bool force_four = false)
{
  LiteralsPlan best = choose_literals(n, all_equal, desc_bytes, stream_bits, force_four);
  if (dict_legal && n >= 2u) {
    const uint32_t one = huf_stream_bytes(dict_bits[0] + dict_bits[1] + dict_bits[2] + dict_bits[3]);
    LiteralsPlan tl{kTreelessLit, 1u, 3u, 3u + one};
    if (n >= 1024u || one >= 1024u || force_four) {
      const uint32_t four = 6u + huf_stream_bytes(dict_bits[0]) + huf_stream_bytes(dict_bits[1]) + huf_stream_bytes(dict_bits[2])
                            + huf_stream_bytes(dict_bits[3]);
      const uint32_t m = n > four ? n : four;
      tl.streams = 4u;
      tl.header_bytes = m < 1024u ? 3u : m < 16384u ? 4u : 5u;
      tl.section_bytes = tl.header_bytes + four;
      if (m >= (1u << 18) || n < 6u)
        tl.section_bytes = 0xFFFFFFFFu;
    }
    if (tl.section_bytes < best.section_bytes || (best.type == (uint32_t)kHufLit && tl.section_bytes == best.section_bytes))
      best = tl;
  }
  return best;
}

// write_literals_header for a plan that may be Treeless (the same header, its type 3)
template <class S>
constexpr uint32_t write_literals_header_dict(const LiteralsPlan& p, uint32_t n, S sink, uint32_t at0)
{
  if (p.type != (uint32_t)kTreelessLit)
    return write_literals_header(p, n, sink, at0);
  LiteralsPlan q = p;
  q.type = kHufLit;
  struct Typed
  {
    S sink;
    uint32_t first;
    constexpr void operator()(uint32_t at, uint8_t b) const { sink(at, at == first ? (uint8_t)(b | 3u) : b); }
  };
  return write_literals_header(q, n, Typed{sink, at0}, at0);
}

// plan_table with the Repeat_Mode candidate: dnorm / dict_log are the dictionary's distribution for this table.
// Where Repeat_Mode wins the encoding table is not built: the caller copies the dictionary's.
template <class H, class Y, class T, class S, class N>
constexpr TablePlan plan_table_dict(uint32_t kind, const H& hist, uint32_t total, Y& symtt, T& states, FseScratch& w, S sink,
                                    uint32_t at0, const N& dnorm, uint32_t dict_log)
{
  const uint32_t nsym = kTableSyms[kind];
  uint32_t used = 0;
  for (uint32_t s = 0; s < nsym; ++s)
    used += hist[s] != 0u;
  if (used >= 2u) {
    const uint32_t dlog = kTableDefaultLog[kind], dsyms = kTableDefaultSyms[kind];
    const uint32_t dcost = kind == kLLTable   ? fse_cost_fix8(hist, nsym, kLLDefault, dsyms, dlog)
                           : kind == kOFTable ? fse_cost_fix8(hist, nsym, kOFDefault, dsyms, dlog)
                                              : fse_cost_fix8(hist, nsym, kMLDefault, dsyms, dlog);
    const uint32_t rcost = fse_cost_fix8(hist, nsym, dnorm, nsym, dict_log);
    const uint32_t log = pick_log(total, used, kTableMaxLog[kind]);
    normalize_counts(hist, nsym, total, log, w.norm);
    const uint32_t own = fse_cost_fix8(hist, nsym, w.norm, nsym, log) + (write_ncount(w.norm, log, NullSink{}, 0u) << 8);
    if (rcost != kCostNever && rcost <= own && !(dcost != kCostNever && dcost <= rcost))
      return TablePlan{kRepeatMode, dict_log, 0u};
  }
  return plan_table(kind, hist, total, symtt, states, w, sink, at0);
}

// ---- the frame header --------------------------------------------------------------------------------------------------
constexpr uint32_t dict_id_bytes(uint32_t dict_id) { return dict_id == 0u ? 0u : dict_id < 256u ? 1u : dict_id < 65536u ? 2u : 4u; }
constexpr uint32_t frame_header_bytes_dict(uint32_t n, uint32_t dict_id) { return frame_header_bytes(n) + dict_id_bytes(dict_id); }

// write_frame_header with the Dictionary_ID in the smallest field that holds it, none for 0
template <class S>
constexpr uint32_t write_frame_header_dict(uint32_t n, bool checksum, uint32_t dict_id, S sink, uint32_t at0)
{
  for (uint32_t b = 0; b < 4u; ++b)
    sink(at0 + b, (uint8_t)(kMagic >> (8u * b)));
  const bool two = n >= 256u;
  const uint32_t idb = dict_id_bytes(dict_id);
  sink(at0 + 4u, (uint8_t)((two ? 1u << 6 : 0u) | (1u << 5) | (checksum ? 1u << 2 : 0u) | (idb == 4u ? 3u : idb)));
  uint32_t at = at0 + 5u;
  for (uint32_t b = 0; b < idb; ++b)
    sink(at++, (uint8_t)(dict_id >> (8u * b)));
  const uint32_t v = two ? n - 256u : n;
  sink(at++, (uint8_t)v);
  if (two)
    sink(at++, (uint8_t)(v >> 8));
  return at - at0;
}

// ---- the scalar encoder --------------------------------------------------------------------------------------------------
// encode_frame against a blob: h / dt are its header and tables (h == nullptr: no dictionary, the frame is
// encode_frame's).  A token's offset may reach into the tail.  -> the frame's bytes, never more than dict_frame_bound(n).
template <class C, class K, class L, class B, class O>
constexpr uint32_t encode_frame_dict(const C& content, uint32_t n, const K& tokens, uint32_t ntok, const L& lits, uint32_t nlit,
                                     bool checksum, const EncBlobHeader* h, const DictTables* dt, EncodeWork& w, B& block, O& out)
{
  const uint32_t dict_id = h ? h->dict_id : 0u;
  const bool entropy = h && h->has_entropy;
  ByteSink<O&> os{out};
  uint32_t at = write_frame_header_dict(n, checksum, dict_id, os, 0u);
  bool all_equal = n >= 2u;
  for (uint32_t i = 1; i < n && all_equal; ++i)
    all_equal = content[i] == content[0];
  uint32_t block_bytes = 0xFFFFFFFFu;
  if (!all_equal && n > 3u) {
    ByteSink<B&> bs{block};
    auto fits = [&](uint32_t end) { return end < n; };
    for (uint32_t s = 0; s < 256u; ++s)
      w.lit_hist[s] = 0;
    for (uint32_t i = 0; i < nlit; ++i)
      w.lit_hist[lits[i]] += 1u;
    uint32_t used = 0;
    bool dict_legal = entropy;
    for (uint32_t s = 0; s < 256u; ++s)
      if (w.lit_hist[s] != 0u) {
        ++used;
        dict_legal = dict_legal && dt->huf[s] != 0u;
      }
    uint32_t desc_bytes = 0, stream_bits[4] = {0, 0, 0, 0}, dict_bits[4] = {0, 0, 0, 0};
    const uint32_t seg = (nlit + 3u) / 4u;
    if (used >= 2u) {
      deflate::build_lengths(w.lit_hist, 256, (int)kHufLogMax, w.huff, w.lens);
      const uint32_t ll = huf_weights_of(w.lens, w.weights);
      huf_codes_of(w.weights, ll >> 16, w.huf, w.ranks);
      desc_bytes = write_weights(w.weights, ll & 0xFFFFu, w.wscratch, ByteSink<uint8_t*>{w.desc}, 0u);
      for (uint32_t i = 0; i < nlit; ++i)
        stream_bits[i / seg] += w.huf[lits[i]] >> 16;
    }
    if (dict_legal)
      for (uint32_t i = 0; i < nlit; ++i)
        dict_bits[i / seg] += dt->huf[lits[i]] >> 16;
    const LiteralsPlan lp = choose_literals_dict(nlit, used == 1u, desc_bytes, stream_bits, dict_legal, dict_bits);
    const bool treeless = lp.type == (uint32_t)kTreelessLit;
    bool ok = fits(lp.section_bytes);
    uint32_t b = 0;
    if (ok) {
      b = write_literals_header_dict(lp, nlit, bs, 0u);
      if (lp.type == (uint32_t)kRawLit) {
        for (uint32_t i = 0; i < nlit; ++i)
          bs(b++, lits[i]);
      } else if (lp.type == (uint32_t)kRleLit) {
        bs(b++, lits[0]);
      } else {
        if (!treeless)
          for (uint32_t i = 0; i < desc_bytes; ++i)
            bs(b++, w.desc[i]);
        const uint32_t nstreams = lp.streams;
        const uint32_t jump = b;
        if (nstreams == 4u)
          b += 6u;
        for (uint32_t k = 0; k < nstreams; ++k) {
          const uint32_t from = nstreams == 1u ? 0u : k * seg;
          const uint32_t to = nstreams == 1u ? nlit : (k == 3u ? nlit : (k + 1u) * seg);
          BitAppender<ByteSink<B&>> ba{bs, b, 0, 0};
          for (uint32_t i = to; i-- > from;) {
            const uint32_t e = treeless ? dt->huf[lits[i]] : w.huf[lits[i]];
            ba.add(e & 0xFFFFu, e >> 16);
          }
          const uint32_t end = ba.close_backward();
          if (nstreams == 4u && k < 3u) {
            bs(jump + 2u * k, (uint8_t)(end - b));
            bs(jump + 2u * k + 1u, (uint8_t)((end - b) >> 8));
          }
          b = end;
        }
      }
    }
    if (ok && ntok == 0u) {
      bs(b++, 0);
    } else if (ok) {
      for (uint32_t t = 0; t < 3u; ++t)
        for (uint32_t s = 0; s < 64u; ++s)
          w.code_hist[t][s] = 0;
      const uint32_t prev0 = h ? h->rep[0] : 0u;
      uint32_t prev = prev0;
      for (uint32_t i = 0; i < ntok; ++i) {
        w.code_hist[kLLTable][ll_code(tokens[i].ll)] += 1u;
        w.code_hist[kOFTable][of_code(offset_value(tokens[i].off, prev, tokens[i].ll))] += 1u;
        w.code_hist[kMLTable][ml_code(tokens[i].ml)] += 1u;
        prev = tokens[i].off;
      }
      ByteSink<uint8_t*> hs{w.seq_head};
      uint32_t hb = write_seq_count(ntok, hs, 0u);
      const uint32_t modes_at = hb++;
      TablePlan tp[3] = {};
      const uint32_t dlogs[3] = {h ? h->ll_log : 0u, h ? h->of_log : 0u, h ? h->ml_log : 0u};
      for (uint32_t t = 0; t < 3u; ++t) {
        if (entropy)
          tp[t] = plan_table_dict(t, w.code_hist[t], ntok, w.symtt[t], w.states[t], w.fse, hs, hb, dt->norm[t], dlogs[t]);
        else
          tp[t] = plan_table(t, w.code_hist[t], ntok, w.symtt[t], w.states[t], w.fse, hs, hb);
        if (tp[t].mode == (uint32_t)kRepeatMode) {
          for (uint32_t s = 0; s < 56u; ++s)
            w.symtt[t][s] = dt->symtt[t][s];
          for (uint32_t s = 0; s < kMaxTableStates; ++s)
            w.states[t][s] = dt->states[t][s];
        }
        hb += tp[t].head_bytes;
      }
      hs(modes_at, (uint8_t)((tp[0].mode << 6) | (tp[1].mode << 4) | (tp[2].mode << 2)));
      ok = fits(b + hb);
      if (ok) {
        for (uint32_t i = 0; i < hb; ++i)
          bs(b++, w.seq_head[i]);
        for (int pass = 0; pass < 2 && ok; ++pass) {
          uint32_t st[3] = {0, 0, 0}, bits = 0;
          BitAppender<ByteSink<B&>> ba{bs, b, 0, 0};
          for (uint32_t i = ntok; i-- > 0u;) {
            const uint32_t pv = i ? tokens[i - 1u].off : prev0;
            const uint32_t ov = offset_value(tokens[i].off, pv, tokens[i].ll);
            const uint32_t code[3] = {ll_code(tokens[i].ll), of_code(ov), ml_code(tokens[i].ml)};
            uint32_t e[3] = {0, 0, 0};
            for (uint32_t t = 0; t < 3u; ++t) {
              if (i + 1u == ntok)
                st[t] = fse_init(w.symtt[t], w.states[t], code[t]);
              else
                e[t] = fse_encode(w.symtt[t], w.states[t], st[t], code[t]);
            }
            const uint32_t field[6][2] = {{e[1] & 0xFFFFu, e[1] >> 16}, {e[2] & 0xFFFFu, e[2] >> 16}, {e[0] & 0xFFFFu, e[0] >> 16},
                                          {tokens[i].ll - kLLBase[code[0]], kLLBits[code[0]]},
                                          {tokens[i].ml - kMLBase[code[2]], kMLBits[code[2]]},
                                          {ov - (1u << code[1]), code[1]}};
            for (uint32_t f = 0; f < 6u; ++f) {
              bits += field[f][1];
              if (pass)
                ba.add(field[f][0], field[f][1]);
            }
          }
          const uint32_t order[3] = {kMLTable, kOFTable, kLLTable};
          for (uint32_t f = 0; f < 3u; ++f) {
            const uint32_t t = order[f];
            bits += tp[t].log;
            if (pass)
              ba.add(st[t] & ((1u << tp[t].log) - 1u), tp[t].log);
          }
          if (!pass)
            ok = fits(b + (bits >> 3) + 1u);
          else
            b = ba.close_backward();
        }
      }
    }
    if (ok && b < n)
      block_bytes = b;
  }
  if (all_equal) {
    at += write_block_header(kRleBlock, n, os, at);
    os(at++, content[0]);
  } else if (block_bytes != 0xFFFFFFFFu) {
    at += write_block_header(kCompressedBlock, block_bytes, os, at);
    for (uint32_t i = 0; i < block_bytes; ++i)
      os(at++, block[i]);
  } else {
    at += write_block_header(kRawBlock, n, os, at);
    for (uint32_t i = 0; i < n; ++i)
      os(at++, content[i]);
  }
  if (checksum) {
    const uint32_t x = (uint32_t)xxh64(content, n, 0);
    for (uint32_t b = 0; b < 4u; ++b)
      os(at++, (uint8_t)(x >> (8u * b)));
  }
  return at;
}

} // namespace zstd
} // namespace hcamd
