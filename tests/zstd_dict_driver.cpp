// zstd_dict_driver.cpp -- a scalar Zstandard frame decoder with dictionaries, composed of
// hipcomp-core_amd/csrc/zstd/zstd_tables.hpp and csrc/zstd_dict/zstd_dict.hpp alone (standard headers, no HIP), for
// tests/test_zstd_dict_cpu.py and tests/zstd_dict_fixtures.py.  It is built with AddressSanitizer and UBSan and runs
// as a process of its own; every dictionary, chunk, blob and output lies in a heap buffer of exactly its size, so a
// read or a write outside one ends the driver.  A dictionary is first digested into the prepared blob of
// zstd_dict.hpp, as the prepare kernel does, and the decode then reads only the blob, as the decode kernel does.
//
//   prepare <cases> <results>  cases: records of u32 length, the dictionary's bytes
//                              results: records of u32 status (0, or 12: refused), u64 blob size, the blob
//   decode <cases> <results>   cases: records of u32 chunk length, u64 capacity, u32 dictionary length (0xFFFFFFFF:
//                              no dictionary), the chunk's bytes, the dictionary's bytes
//                              results: records of u32 verdict (1: decoded), u64 size, u32 matches that begin in the
//                              dictionary, u32 of those that continue into the output, u32 forms of the first block
//                              of the first frame (1: Treeless literals, 2 / 4 / 8: Repeat_Mode for LL / OF / ML),
//                              the decoded bytes
//   sizes <cases> <results>    the size query on the same cases: records of u64 size (0: refused)
//   preparedsize <dict_bytes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zstd/zstd_tables.hpp"
#include "zstd_dict/zstd_dict.hpp"

using namespace hcamd::zstd;

namespace {

struct Tables
{
  FseEntry ll[1 << kLLLogMax], of[1 << kOFLogMax], ml[1 << kMLLogMax], wt[1 << kWeightLogMax];
  uint32_t ll_log = 0, of_log = 0, ml_log = 0;
  uint16_t huf[1 << kHufLogMax];
  uint32_t huf_log = 0;
  bool have_huf = false, have_fse = false;
  int16_t norm[256];
  uint16_t next[256];
  uint8_t weights[256], sorted[256];
  uint32_t count[kHufLogMax + 2];
};

struct Counts
{
  uint32_t in_dict = 0, crossing = 0, first_block = 0;
  bool first_seen = false;
};

// the blob of p[0, n) in a heap buffer of exactly prepared_bytes(n), or empty: refused
std::vector<uint8_t> prepare(const uint8_t* p, uint32_t n)
{
  static Tables t;
  const DictLayout d = parse_dictionary(p, n, t.weights, t.norm, t.wt, t.next);
  if (!d.ok)
    return {};
  std::vector<uint8_t> blob(prepared_bytes(n), 0);
  PreparedHeader h{kPreparedMagic, kPreparedVersion, 1, d.dict_id, d.formatted ? 1u : 0u, 0, 0, 0, 0, {d.rep[0], d.rep[1], d.rep[2]},
                   kPreparedContent, d.content_size, (uint32_t)blob.size(), 0};
  if (d.formatted) {
    const HufDesc hd = read_huf_weights(p + d.huf_at, n - d.huf_at, t.weights, t.norm, t.wt, t.next);
    huf_sort(t.weights, hd.nsym, t.count, t.sorted);
    uint16_t* huf = reinterpret_cast<uint16_t*>(blob.data() + kPreparedHuf);
    for (uint32_t e = 0; e < (1u << hd.log); ++e)
      huf[e] = (uint16_t)huf_entry(e, t.count, t.sorted, hd.log);
    const NCount of = read_ncount(p + d.of_at, n - d.of_at, t.norm, kOFSymMax, kOFLogMax);
    fse_build(t.norm, of.nsym, of.log, reinterpret_cast<FseEntry*>(blob.data() + kPreparedOF), t.next);
    const NCount ml = read_ncount(p + d.ml_at, n - d.ml_at, t.norm, kMLSymMax, kMLLogMax);
    fse_build(t.norm, ml.nsym, ml.log, reinterpret_cast<FseEntry*>(blob.data() + kPreparedML), t.next);
    const NCount ll = read_ncount(p + d.ll_at, n - d.ll_at, t.norm, kLLSymMax, kLLLogMax);
    fse_build(t.norm, ll.nsym, ll.log, reinterpret_cast<FseEntry*>(blob.data() + kPreparedLL), t.next);
    h.ll_log = ll.log;
    h.ml_log = ml.log;
    h.of_log = of.log;
    h.huf_log = hd.log;
  }
  if (d.content_size)
    memcpy(blob.data() + kPreparedContent, p + d.content_at, d.content_size);
  memcpy(blob.data(), &h, sizeof h);
  return blob;
}

// a frame's view of the blob (null: no dictionary)
struct Dict
{
  const uint8_t* blob = nullptr;
  PreparedHeader h{};
  const uint8_t* content() const { return blob + kPreparedContent; }
};

bool open_dict(const uint8_t* blob, Dict& d)
{
  d = Dict{};
  d.h.rep[0] = 1;
  d.h.rep[1] = 4;
  d.h.rep[2] = 8;
  if (!blob)
    return true;
  d.blob = blob;
  memcpy(&d.h, blob, sizeof d.h);
  return d.h.magic == kPreparedMagic && d.h.version == kPreparedVersion && d.h.valid == 1;
}

// every frame starts from the dictionary's tables
void start_frame(Tables& t, const Dict& d)
{
  t.have_huf = t.have_fse = false;
  if (d.blob && d.h.has_entropy) {
    memcpy(t.ll, d.blob + kPreparedLL, sizeof t.ll);
    memcpy(t.ml, d.blob + kPreparedML, sizeof t.ml);
    memcpy(t.of, d.blob + kPreparedOF, sizeof t.of);
    memcpy(t.huf, d.blob + kPreparedHuf, sizeof t.huf);
    t.ll_log = d.h.ll_log;
    t.ml_log = d.h.ml_log;
    t.of_log = d.h.of_log;
    t.huf_log = d.h.huf_log;
    t.have_huf = t.have_fse = true;
  }
}

bool seq_table(uint32_t mode, const uint8_t* p, uint32_t n, uint32_t& at, FseEntry* table, uint32_t& log, const int16_t* def,
               uint32_t def_syms, uint32_t def_log, uint32_t max_sym, uint32_t max_log, bool have_previous, Tables& t)
{
  switch (mode) {
  case kPredefined:
    for (uint32_t s = 0; s < def_syms; ++s)
      t.norm[s] = def[s];
    fse_build(t.norm, def_syms, def_log, table, t.next);
    log = def_log;
    return true;
  case kRleMode:
    if (at >= n || p[at] > max_sym)
      return false;
    fse_build_rle(table, p[at]);
    log = 0;
    at += 1;
    return true;
  case kFseMode: {
    const NCount nc = read_ncount(p + at, n - at, t.norm, max_sym, max_log);
    if (!nc.ok)
      return false;
    fse_build(t.norm, nc.nsym, nc.log, table, t.next);
    log = nc.log;
    at += nc.bytes;
    return true;
  }
  default:
    return have_previous;
  }
}

bool huf_stream(const uint8_t* p, uint32_t n, uint8_t* dst, uint32_t count, const Tables& t)
{
  BackBits<const uint8_t*> bs{};
  if (!bs.init(p, n))
    return false;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t e = t.huf[bs.peek(t.huf_log)];
    bs.left -= (int32_t)(e & 0xFFu);
    if (bs.left < 0)
      return false;
    dst[i] = (uint8_t)(e >> 8);
  }
  return bs.left == 0;
}

// -> false: refused.  out == nullptr: the size query (nothing stored, offsets still checked).
bool decode_block(const uint8_t* p, uint32_t n, uint8_t* out, uint64_t cap, uint64_t frame_start, uint64_t& produced,
                  Tables& t, SeqState& st, std::vector<uint8_t>& lits, const Dict& dict, Counts& counts)
{
  const LitHeader lh = parse_literals_header(p, n);
  if (!lh.ok)
    return false;
  uint32_t forms = lh.type == kTreelessLit ? 1u : 0u;
  lits.assign(lh.regen, 0);
  const uint8_t* body = p + lh.header_bytes;
  if (lh.regen == 0 && lh.type <= kRleLit) {
    // nothing to copy or fill
  } else if (lh.type == kRawLit) {
    memcpy(lits.data(), body, lh.regen);
  } else if (lh.type == kRleLit) {
    memset(lits.data(), body[0], lh.regen);
  } else {
    uint32_t at = 0;
    if (lh.type == kHufLit) {
      const HufDesc d = read_huf_weights(body, lh.comp, t.weights, t.norm, t.wt, t.next);
      if (!d.ok)
        return false;
      huf_sort(t.weights, d.nsym, t.count, t.sorted);
      for (uint32_t e = 0; e < (1u << d.log); ++e)
        t.huf[e] = (uint16_t)huf_entry(e, t.count, t.sorted, d.log);
      t.huf_log = d.log;
      t.have_huf = true;
      at = d.bytes;
    } else if (!t.have_huf) {
      return false;
    }
    if (lh.streams == 1) {
      if (!huf_stream(body + at, lh.comp - at, lits.data(), lh.regen, t))
        return false;
    } else {
      uint32_t size[4];
      if (!huf_jump_table(body + at, lh.comp - at, size))
        return false;
      const uint32_t seg = (lh.regen + 3u) / 4u;
      if (3u * seg > lh.regen)
        return false;
      uint32_t src = at + 6u;
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t cnt = j < 3 ? seg : lh.regen - 3u * seg;
        if (!huf_stream(body + src, size[j], lits.data() + j * seg, cnt, t))
          return false;
        src += size[j];
      }
    }
  }
  const uint32_t lit_bytes = lh.header_bytes + lh.comp;
  const SeqHeader sh = parse_sequences_header(p + lit_bytes, n - lit_bytes);
  if (!sh.ok)
    return false;
  uint32_t at = lit_bytes + sh.header_bytes;
  uint32_t litpos = 0;
  const uint64_t content_size = dict.blob ? dict.h.content_size : 0;
  if (sh.nseq) {
    forms |= (sh.ll_mode == kRepeatMode ? 2u : 0u) | (sh.of_mode == kRepeatMode ? 4u : 0u) | (sh.ml_mode == kRepeatMode ? 8u : 0u);
    if (!seq_table(sh.ll_mode, p, n, at, t.ll, t.ll_log, kLLDefault, 36, kLLDefaultLog, kLLSymMax, kLLLogMax, t.have_fse, t) ||
        !seq_table(sh.of_mode, p, n, at, t.of, t.of_log, kOFDefault, 29, kOFDefaultLog, kOFSymMax, kOFLogMax, t.have_fse, t) ||
        !seq_table(sh.ml_mode, p, n, at, t.ml, t.ml_log, kMLDefault, 53, kMLDefaultLog, kMLSymMax, kMLLogMax, t.have_fse, t))
      return false;
    t.have_fse = true;
    BackBits<const uint8_t*> bs{};
    if (!bs.init(p + at, n - at))
      return false;
    st.ll = bs.read(t.ll_log);
    st.of = bs.read(t.of_log);
    st.ml = bs.read(t.ml_log);
    if (bs.left < 0)
      return false;
    for (uint32_t k = 0; k < sh.nseq; ++k) {
      const Sequence q = decode_sequence(bs, st, t.ll, t.of, t.ml, k + 1 == sh.nseq);
      if (bs.left < 0)
        return false;
      if (q.ll > lh.regen - litpos || (uint64_t)q.ll + q.ml > cap - produced)
        return false;
      const uint64_t pos = produced + q.ll - frame_start; // of the match, in the frame
      if (!offset_in_history(q.off, pos, content_size))
        return false;
      if (q.off > pos) {
        counts.in_dict += 1;
        counts.crossing += q.ml > q.off - pos;
      }
      if (out) {
        if (q.ll)
          memcpy(out + produced, lits.data() + litpos, q.ll);
        uint8_t* dst = out + produced + q.ll;
        const uint64_t v0 = content_size + pos - q.off;
        for (uint32_t i = 0; i < q.ml; ++i)
          dst[i] = history_at(dict.blob ? dict.content() : out, content_size, out + frame_start, v0 + (q.off < q.ml ? i % q.off : i));
      }
      litpos += q.ll;
      produced += (uint64_t)q.ll + q.ml;
    }
    if (bs.left != 0)
      return false;
  }
  const uint32_t tail = lh.regen - litpos;
  if (tail > cap - produced)
    return false;
  if (out && tail)
    memcpy(out + produced, lits.data() + litpos, tail);
  produced += tail;
  if (!counts.first_seen) {
    counts.first_seen = true;
    counts.first_block = forms;
  }
  return true;
}

bool decode_chunk(const uint8_t* p, uint64_t n, uint8_t* out, uint64_t cap, uint64_t& produced, const uint8_t* blob, Counts& counts)
{
  static Tables t;
  std::vector<uint8_t> lits;
  uint64_t at = 0;
  produced = 0;
  Dict dict;
  if (!open_dict(blob, dict))
    return false;
  while (at < n) {
    const FrameHeader fh = parse_frame_header(p + at, n - at, true);
    if (fh.kind == kNoFrame)
      return false;
    if (fh.kind == kSkippableFrame) {
      at += fh.skip_bytes;
      continue;
    }
    if (!dict_id_accepted(fh.dict_id, dict.blob ? dict.h.dict_id : 0))
      return false;
    at += fh.header_bytes;
    const uint64_t frame_start = produced;
    SeqState st{0, 0, 0, {dict.h.rep[0], dict.h.rep[1], dict.h.rep[2]}};
    start_frame(t, dict);
    for (;;) {
      const BlockHeader bh = parse_block_header(p + at, n - at);
      if (!bh.ok)
        return false;
      at += 3;
      if (bh.type == kCompressedBlock) {
        if (bh.size >= kBlockMax)
          return false;
        if (!decode_block(p + at, bh.size, out, cap, frame_start, produced, t, st, lits, dict, counts))
          return false;
      } else {
        counts.first_seen = true;
        if (bh.size > cap - produced)
          return false;
        if (out && bh.size) {
          if (bh.type == kRawBlock)
            memcpy(out + produced, p + at, bh.size);
          else
            memset(out + produced, p[at], bh.size);
        }
        produced += bh.size;
      }
      at += bh.comp_bytes;
      if (bh.last)
        break;
    }
    if (fh.has_size && produced - frame_start != fh.content_size)
      return false;
    if (fh.checksum) {
      if (n - at < 4)
        return false;
      if (out && (uint32_t)xxh64(out + frame_start, produced - frame_start, 0) != (uint32_t)read_le(p, at, 4))
        return false;
      at += 4;
    }
  }
  return true;
}

// the size query: the declared sizes where every frame declares one (headers walked with the ID rule)
uint64_t query_size(const uint8_t* p, uint64_t n, const uint8_t* blob)
{
  uint64_t at = 0, total = 0;
  bool all_declared = true;
  Dict dict;
  if (!open_dict(blob, dict))
    return 0;
  while (at < n && all_declared) {
    const FrameHeader fh = parse_frame_header(p + at, n - at, true);
    if (fh.kind == kNoFrame)
      return 0;
    if (fh.kind == kSkippableFrame) {
      at += fh.skip_bytes;
      continue;
    }
    if (!dict_id_accepted(fh.dict_id, dict.blob ? dict.h.dict_id : 0))
      return 0;
    at += fh.header_bytes;
    if (!fh.has_size) {
      all_declared = false;
      break;
    }
    total += fh.content_size;
    for (;;) {
      const BlockHeader bh = parse_block_header(p + at, n - at);
      if (!bh.ok)
        return 0;
      at += 3u + bh.comp_bytes;
      if (bh.last)
        break;
    }
    if (fh.checksum) {
      if (n - at < 4)
        return 0;
      at += 4;
    }
  }
  if (all_declared)
    return total;
  uint64_t produced = 0;
  Counts counts;
  return decode_chunk(p, n, nullptr, ~0ull, produced, blob, counts) ? produced : 0;
}

std::vector<uint8_t> slurp(const char* path)
{
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0)
    v.insert(v.end(), buf, buf + got);
  fclose(f);
  return v;
}

uint8_t* heap_copy(const uint8_t* p, size_t n)
{
  uint8_t* q = (uint8_t*)malloc(n ? n : 1);
  if (n)
    memcpy(q, p, n);
  return q;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc == 3 && !strcmp(argv[1], "preparedsize")) {
    printf("%llu\n", (unsigned long long)prepared_bytes(strtoull(argv[2], 0, 10)));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "prepare")) {
    const std::vector<uint8_t> all = slurp(argv[2]);
    FILE* f = fopen(argv[3], "wb");
    size_t at = 0;
    while (at + 4 <= all.size()) {
      uint32_t len;
      memcpy(&len, &all[at], 4);
      at += 4;
      uint8_t* in = heap_copy(all.data() + at, len);
      at += len;
      const std::vector<uint8_t> blob = prepare(in, len);
      const uint32_t status = blob.empty() ? 12u : 0u;
      const uint64_t size = blob.size();
      fwrite(&status, 4, 1, f);
      fwrite(&size, 8, 1, f);
      if (!blob.empty())
        fwrite(blob.data(), 1, blob.size(), f);
      free(in);
    }
    fclose(f);
    return 0;
  }
  if (argc == 4 && (!strcmp(argv[1], "decode") || !strcmp(argv[1], "sizes"))) {
    const bool sizes = argv[1][0] == 's';
    const std::vector<uint8_t> all = slurp(argv[2]);
    FILE* f = fopen(argv[3], "wb");
    size_t at = 0;
    while (at + 16 <= all.size()) {
      uint32_t len, dlen;
      uint64_t cap;
      memcpy(&len, &all[at], 4);
      memcpy(&cap, &all[at + 4], 8);
      memcpy(&dlen, &all[at + 12], 4);
      at += 16;
      uint8_t* in = heap_copy(all.data() + at, len);
      at += len;
      const bool with_dict = dlen != 0xFFFFFFFFu;
      bool dict_ok = true;
      uint8_t* blob = nullptr;
      if (with_dict) {
        uint8_t* dict = heap_copy(all.data() + at, dlen);
        at += dlen;
        const std::vector<uint8_t> b = prepare(dict, dlen);
        free(dict);
        dict_ok = !b.empty();
        if (dict_ok)
          blob = heap_copy(b.data(), b.size());
      }
      if (sizes) {
        const uint64_t s = dict_ok ? query_size(in, len, blob) : 0;
        fwrite(&s, 8, 1, f);
      } else {
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        uint64_t produced = 0;
        Counts counts;
        const uint32_t ok = dict_ok && decode_chunk(in, len, out, cap, produced, blob, counts) ? 1u : 0u;
        if (!ok)
          produced = 0;
        fwrite(&ok, 4, 1, f);
        fwrite(&produced, 8, 1, f);
        fwrite(&counts.in_dict, 4, 1, f);
        fwrite(&counts.crossing, 4, 1, f);
        fwrite(&counts.first_block, 4, 1, f);
        fwrite(out, 1, produced, f);
        free(out);
      }
      free(blob);
      free(in);
    }
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: %s prepare|decode|sizes <cases> <results> | preparedsize <dict_bytes>\n", argv[0]);
  return 2;
}
