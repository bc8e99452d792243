// zstd_tables_driver.cpp -- a scalar Zstandard frame decoder composed of hipcomp-core_amd/csrc/zstd/zstd_tables.hpp
// and xxh64_math.hpp alone (standard headers, no HIP), for tests/test_zstd_tables_cpu.py.  It is built with
// AddressSanitizer and UBSan and runs as a process of its own; every chunk is decoded from a heap buffer of
// exactly its length into a heap buffer of exactly its capacity, so a read or a write outside either ends the
// driver.  The kernel (zstd_kernels.hip) composes the same functions in the same order.
//
//   decode <cases> <results>   cases: records of u32 length, u64 capacity, the chunk's bytes
//                              results: records of u32 verdict (1: decoded), u64 size, the decoded bytes
//   sizes <cases> <results>    the size query: records of u64 size (0: refused)
//   xxh64 <file>               XXH64, seed 0, of the file in hexadecimal
//   tempsize <chunks> <max> <waves>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zstd/zstd_tables.hpp"
#include "zstd/zstd_sizing.hpp"

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

// one of the three sequence tables by its mode; `at` advances over what the mode reads from p[0, n)
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
    if (dst)
      dst[i] = (uint8_t)(e >> 8);
  }
  return bs.left == 0;
}

// -> false: refused.  out == nullptr: the size query (nothing stored, offsets still checked).
bool decode_block(const uint8_t* p, uint32_t n, uint8_t* out, uint64_t cap, uint64_t frame_start, uint64_t& produced,
                  Tables& t, SeqState& st, std::vector<uint8_t>& lits)
{
  const LitHeader lh = parse_literals_header(p, n);
  if (!lh.ok)
    return false;
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
  if (sh.nseq) {
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
      if (q.off > produced + q.ll - frame_start)
        return false;
      if (out) {
        if (q.ll)
          memcpy(out + produced, lits.data() + litpos, q.ll);
        uint8_t* dst = out + produced + q.ll;
        for (uint32_t i = 0; i < q.ml; ++i)
          dst[i] = dst[(int64_t)i - (int64_t)q.off];
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
  return true;
}

bool decode_chunk(const uint8_t* p, uint64_t n, uint8_t* out, uint64_t cap, uint64_t& produced)
{
  static Tables t;
  std::vector<uint8_t> lits;
  uint64_t at = 0;
  produced = 0;
  while (at < n) {
    const FrameHeader fh = parse_frame_header(p + at, n - at);
    if (fh.kind == kNoFrame)
      return false;
    if (fh.kind == kSkippableFrame) {
      at += fh.skip_bytes;
      continue;
    }
    at += fh.header_bytes;
    const uint64_t frame_start = produced;
    SeqState st{0, 0, 0, {1, 4, 8}};
    t.have_huf = t.have_fse = false;
    for (;;) {
      const BlockHeader bh = parse_block_header(p + at, n - at);
      if (!bh.ok)
        return false;
      at += 3;
      if (bh.type == kCompressedBlock) {
        if (bh.size >= kBlockMax)
          return false;
        if (!decode_block(p + at, bh.size, out, cap, frame_start, produced, t, st, lits))
          return false;
      } else {
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

// the size query: the declared sizes where every frame declares one (headers walked, nothing decoded)
uint64_t query_size(const uint8_t* p, uint64_t n)
{
  uint64_t at = 0, total = 0;
  bool all_declared = true;
  while (at < n && all_declared) {
    const FrameHeader fh = parse_frame_header(p + at, n - at);
    if (fh.kind == kNoFrame)
      return 0;
    if (fh.kind == kSkippableFrame) {
      at += fh.skip_bytes;
      continue;
    }
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
  return decode_chunk(p, n, nullptr, ~0ull, produced) ? produced : 0;
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

} // namespace

int main(int argc, char** argv)
{
  if (argc == 3 && !strcmp(argv[1], "xxh64")) {
    const std::vector<uint8_t> v = slurp(argv[2]);
    uint8_t* heap = (uint8_t*)malloc(v.size() ? v.size() : 1);
    if (!v.empty())
      memcpy(heap, v.data(), v.size());
    printf("%016llx\n", (unsigned long long)xxh64((const uint8_t*)heap, v.size(), 0));
    free(heap);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "tempsize")) {
    printf("%llu\n", (unsigned long long)temp_bytes(strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10), strtoull(argv[4], 0, 10)));
    return 0;
  }
  if (argc == 4 && (!strcmp(argv[1], "decode") || !strcmp(argv[1], "sizes"))) {
    const bool sizes = argv[1][0] == 's';
    const std::vector<uint8_t> all = slurp(argv[2]);
    FILE* f = fopen(argv[3], "wb");
    size_t at = 0;
    while (at + 12 <= all.size()) {
      uint32_t len;
      uint64_t cap;
      memcpy(&len, &all[at], 4);
      memcpy(&cap, &all[at + 4], 8);
      at += 12;
      uint8_t* in = (uint8_t*)malloc(len ? len : 1);
      memcpy(in, all.data() + at, len);
      at += len;
      if (sizes) {
        const uint64_t s = query_size(in, len);
        fwrite(&s, 8, 1, f);
      } else {
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        uint64_t produced = 0;
        const uint32_t ok = decode_chunk(in, len, out, cap, produced) ? 1u : 0u;
        if (!ok)
          produced = 0;
        fwrite(&ok, 4, 1, f);
        fwrite(&produced, 8, 1, f);
        fwrite(out, 1, produced, f);
        free(out);
      }
      free(in);
    }
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: %s decode|sizes <cases> <results> | xxh64 <file> | tempsize <chunks> <max> <waves>\n", argv[0]);
  return 2;
}
