// CPU driver of csrc/zstd_dict_compress/zstd_dict_codes.hpp: the header the kernels include, composed into the
// scalar prepare and the scalar encoder against a blob.  A stand-alone program, built with the sanitizers by
// tests/zstd_dict_codes_fixtures.py and never loaded into Python.
//
//   zstd_dict_codes_driver prepare <cases> <results>
//       cases:   per dictionary  u32 bytes | the dictionary
//       results: per dictionary  u32 status (0 prepared, 1 refused) | u64 size | the blob (refused: its 64-byte header)
//   zstd_dict_codes_driver encode <cases> <results>
//       cases:   per chunk  u32 flags (1: checksum, 2: a dictionary follows) | u32 dictionary bytes | u32 n | u32 tokens |
//                the dictionary | the content | tokens x (u32 ll, u32 ml, u32 offset)
//       results: per chunk  u32 size | the frame   (size 0: the dictionary was refused)
//   zstd_dict_codes_driver size <dict_bytes>          prints enc_prepared_bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "zstd_dict_compress/zstd_dict_codes.hpp"

using namespace hcamd::zstd;

static std::vector<uint8_t> slurp(const char* path)
{
  std::vector<uint8_t> out;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0)
    out.insert(out.end(), buf, buf + n);
  fclose(f);
  return out;
}

static uint32_t u32_at(const std::vector<uint8_t>& v, size_t at)
{
  if (at + 4 > v.size()) {
    fprintf(stderr, "a truncated case file\n");
    exit(2);
  }
  uint32_t x;
  memcpy(&x, &v[at], 4);
  return x;
}

// exact-size heap copies, so that the sanitizer sees every byte past an end
static std::unique_ptr<uint8_t[]> exact(const uint8_t* from, size_t n)
{
  std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
  if (n)
    memcpy(p.get(), from, n);
  return p;
}

int main(int argc, char** argv)
{
  if (argc == 3 && !strcmp(argv[1], "size")) {
    printf("%llu\n", (unsigned long long)enc_prepared_bytes(strtoull(argv[2], 0, 10)));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "prepare")) {
    const std::vector<uint8_t> all = slurp(argv[2]);
    FILE* f = fopen(argv[3], "wb");
    if (!f)
      return 2;
    auto work = std::make_unique<PrepareWork>();
    for (size_t at = 0; at < all.size();) {
      const uint32_t n = u32_at(all, at);
      at += 4;
      if (at + n > all.size())
        return 2;
      const auto dict = exact(&all[at], n);
      at += n;
      const uint64_t size = enc_prepared_bytes(n);
      std::unique_ptr<uint8_t[]> blob(new uint8_t[size]);
      const bool ok = prepare_scalar(dict.get(), n, *work, blob.get());
      const uint32_t status = ok ? 0u : 1u;
      const uint64_t written = ok ? size : sizeof(EncBlobHeader);
      fwrite(&status, 4, 1, f);
      fwrite(&written, 8, 1, f);
      fwrite(blob.get(), 1, written, f);
    }
    fclose(f);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "encode")) {
    const std::vector<uint8_t> all = slurp(argv[2]);
    FILE* f = fopen(argv[3], "wb");
    if (!f)
      return 2;
    auto pwork = std::make_unique<PrepareWork>();
    auto work = std::make_unique<EncodeWork>();
    for (size_t at = 0; at < all.size();) {
      const uint32_t flags = u32_at(all, at), dn = u32_at(all, at + 4), n = u32_at(all, at + 8), ntok = u32_at(all, at + 12);
      at += 16;
      if (at + dn + n + 12ull * ntok > all.size() || n > kDictEncMaxChunk)
        return 2;
      const auto dict = exact(&all[at], dn);
      at += dn;
      const auto content = exact(&all[at], n);
      at += n;
      std::vector<Token> tokens(ntok);
      for (uint32_t i = 0; i < ntok; ++i, at += 12)
        tokens[i] = Token{u32_at(all, at), u32_at(all, at + 4), u32_at(all, at + 8)};
      const bool with = (flags & 2u) != 0;
      std::unique_ptr<uint8_t[]> blob(new uint8_t[enc_prepared_bytes(dn)]);
      uint32_t size = 0;
      if (!with || prepare_scalar(dict.get(), dn, *pwork, blob.get())) {
        EncBlobHeader h{};
        auto tables = std::make_unique<DictTables>();
        uint32_t content_size = 0;
        const uint8_t* dict_content = nullptr;
        if (with) {
          memcpy(&h, blob.get(), sizeof h);
          memcpy(tables.get(), blob.get() + kEncBlobTables, sizeof(DictTables));
          content_size = h.content_size;
          dict_content = dict.get() + (dn - content_size);
        }
        // the tokens are matches of content ++ chunk (the decoder's history), their literals gathered
        std::vector<uint8_t> lits;
        uint32_t pos = 0;
        for (const Token& t : tokens) {
          if (t.ml < 3 || t.off < 1 || t.off > 65535u || (uint64_t)t.off > (uint64_t)pos + t.ll + content_size
              || (uint64_t)pos + t.ll + t.ml > n) {
            fprintf(stderr, "a token outside the history\n");
            return 2;
          }
          lits.insert(lits.end(), content.get() + pos, content.get() + pos + t.ll);
          pos += t.ll;
          for (uint32_t k = 0; k < t.ml; ++k, ++pos) {
            const int64_t from = (int64_t)pos - t.off;
            const uint8_t b = from >= 0 ? content[from] : dict_content[content_size + from];
            if (content[pos] != b) {
              fprintf(stderr, "a token that is no match\n");
              return 2;
            }
          }
        }
        lits.insert(lits.end(), content.get() + pos, content.get() + n);
        const auto lit_heap = exact(lits.data(), lits.size());
        std::unique_ptr<Token[]> tok_heap(new Token[ntok ? ntok : 1]);
        for (uint32_t i = 0; i < ntok; ++i)
          tok_heap[i] = tokens[i];
        std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
        std::unique_ptr<uint8_t[]> out(new uint8_t[dict_frame_bound(n)]);
        const uint8_t* cp = content.get();
        const uint8_t* lp = lit_heap.get();
        const Token* tp = tok_heap.get();
        uint8_t* bp = block.get();
        uint8_t* op = out.get();
        size = encode_frame_dict(cp, n, tp, ntok, lp, (uint32_t)lits.size(), (flags & 1u) != 0, with ? &h : nullptr,
                                 with ? tables.get() : nullptr, *work, bp, op);
        if (size > dict_frame_bound(n))
          return 3;
        fwrite(&size, 4, 1, f);
        fwrite(out.get(), 1, size, f);
      } else {
        fwrite(&size, 4, 1, f);
      }
    }
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: %s prepare|encode <cases> <results> | size <dict_bytes>\n", argv[0]);
  return 2;
}
