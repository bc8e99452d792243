// The host logic of the gzip / zlib / BGZF entry points (hipcomp-core_amd/csrc/gzip/gzip_frame.hpp and
// adler32_math.hpp) on the CPU, for tests/test_gzip_frame_cpu.py (g++, standard headers only; the test builds it
// with -fsanitize=address,undefined and runs it as a process of its own).
//   gzip_frame_driver parse WRAPPER CASES      CASES holds [u32 length][bytes] records: each is copied into a heap
//                                              buffer of exactly its length and parsed there, one line each:
//                                              ok payload_at payload_bytes check isize
//   gzip_frame_driver header WRAPPER MEMBER    the header bytes in hex, for a member of MEMBER bytes
//   gzip_frame_driver trailer WRAPPER CHECK ISIZE
//   gzip_frame_driver eof                      the BGZF end-of-file block in hex
//   gzip_frame_driver bound N WRAPPER          max_member_bytes
//   gzip_frame_driver adler FILE               adler32_of, and the same from 16-byte blocks as a lane of the kernel
//                                              takes them (from every start offset 0..15)
//   gzip_frame_driver parts FILE LEN...        the value joined from the pieces' sums
//   gzip_frame_driver split FILE CAP           count, where the walk stopped, the offsets
#include "adler32_math.hpp"
#include "gzip_frame.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace hcamd;

static_assert(gzipframe::max_member_bytes(65536, gzipframe::kGzip) == 65546 + 18, "bound");
static_assert(gzipframe::max_member_bytes(65280, gzipframe::kBgzf) <= 65536, "a stored BGZF block fits BSIZE");
static_assert(gzipframe::kBgzfEof[16] == 27 && sizeof(gzipframe::kBgzfEof) == 28, "end-of-file block");

static std::vector<uint8_t> read_file(const char* path)
{
  std::vector<uint8_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f)
    std::exit(2);
  uint8_t buf[65536];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0)
    v.insert(v.end(), buf, buf + got);
  std::fclose(f);
  return v;
}

static uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// As a lane of gzip_kernels.hip: `lead` single bytes, whole 16-byte blocks with a reduction every 344, single bytes
static uint32_t adler_blocked(const uint8_t* p, size_t n, size_t lead)
{
  lead = lead < n ? lead : n;
  uint32_t a = 0, b = 0, left = adler32::kBlocksPerReduce - 3;
  adler32::update_bytes(a, b, p, lead);
  size_t i = lead;
  for (; i + 16 <= n; i += 16) {
    adler32::update_16(a, b, le32(p + i), le32(p + i + 4), le32(p + i + 8), le32(p + i + 12));
    if (--left == 0) {
      a %= adler32::kMod;
      b %= adler32::kMod;
      left = adler32::kBlocksPerReduce - 3;
    }
  }
  adler32::update_bytes(a, b, p + i, n - i);
  const adler32::Piece piece{a % adler32::kMod, b % adler32::kMod};
  return adler32::finish(piece.a, adler32::b_share(piece, 0), n);
}

int main(int argc, char** argv)
{
  if (argc < 2)
    return 2;
  const std::string cmd = argv[1];
  if (cmd == "parse" && argc == 4) {
    const int wrapper = std::atoi(argv[2]);
    const std::vector<uint8_t> all = read_file(argv[3]);
    size_t at = 0;
    while (at + 4 <= all.size()) {
      const size_t n = le32(all.data() + at);
      at += 4;
      if (n > all.size() - at)
        return 3;
      std::unique_ptr<uint8_t[]> exact(new uint8_t[n]);   // exactly n bytes: a read at p[n] is a heap overflow
      if (n)
        std::memcpy(exact.get(), all.data() + at, n);
      at += n;
      const gzipframe::Member m = gzipframe::parse_member(exact.get(), n, wrapper);
      std::printf("%d %zu %zu %u %u\n", m.ok ? 1 : 0, m.payload_at, m.payload_bytes, m.check, m.isize);
    }
  } else if (cmd == "header" && argc == 4) {
    const int w = std::atoi(argv[2]);
    for (uint32_t k = 0; k < gzipframe::header_bytes(w); ++k)
      std::printf("%02x", gzipframe::header_byte(w, k, (uint32_t)std::strtoul(argv[3], nullptr, 0)));
    std::printf("\n");
  } else if (cmd == "trailer" && argc == 5) {
    const int w = std::atoi(argv[2]);
    for (uint32_t k = 0; k < gzipframe::trailer_bytes(w); ++k)
      std::printf("%02x", gzipframe::trailer_byte(w, k, (uint32_t)std::strtoul(argv[3], nullptr, 0),
                                                  (uint32_t)std::strtoul(argv[4], nullptr, 0)));
    std::printf("\n");
  } else if (cmd == "eof") {
    for (uint8_t v : gzipframe::kBgzfEof)
      std::printf("%02x", v);
    std::printf("\n");
  } else if (cmd == "bound" && argc == 4) {
    std::printf("%zu\n", gzipframe::max_member_bytes(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3])));
  } else if (cmd == "adler" && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    std::printf("%u", adler32::adler32_of(d.data(), d.size()));
    for (size_t lead = 0; lead < 16; ++lead)
      std::printf(" %u", adler_blocked(d.data(), d.size(), lead));
    std::printf("\n");
  } else if (cmd == "parts" && argc >= 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    uint64_t at = 0, total = 0;
    for (int k = 3; k < argc; ++k)
      total += std::strtoull(argv[k], nullptr, 0);
    if (total != d.size())
      return 3;
    uint32_t sum_a = 0, sum_b = 0;   // reduced at every step here: the number of pieces has no bound
    for (int k = 3; k < argc; ++k) {
      const uint64_t len = std::strtoull(argv[k], nullptr, 0);
      const adler32::Piece piece = adler32::piece_of(d.data() + at, len);
      sum_a = (sum_a + piece.a) % adler32::kMod;
      sum_b = (sum_b + adler32::b_share(piece, total - at - len)) % adler32::kMod;
      at += len;
    }
    std::printf("%u\n", adler32::finish(sum_a, sum_b, total));
  } else if (cmd == "split" && argc == 4) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    const size_t cap = std::strtoull(argv[3], nullptr, 0);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[d.size()]);
    if (!d.empty())
      std::memcpy(exact.get(), d.data(), d.size());
    std::unique_ptr<size_t[]> offsets(new size_t[cap]);
    size_t count = 0;
    const size_t stopped = gzipframe::bgzf_split(exact.get(), d.size(), offsets.get(), cap, &count);
    std::printf("%zu %zu", count, stopped);
    for (size_t k = 0; k < count; ++k)
      std::printf(" %zu", offsets[k]);
    std::printf("\n");
  } else {
    return 2;
  }
  return 0;
}
