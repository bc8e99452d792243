// The CRC-32 math of the high-level managers' checksums (hipcomp-core_amd/csrc/crc32_math.hpp) on the CPU,
// for tests/test_crc32_cpu.py (g++, standard headers only).
//   crc32_driver tables                      the 16 slice tables, 256 hex words a line
//   crc32_driver crc FILE                    bytewise CRC, slice-by-16 CRC (from every start offset 0..15)
//   crc32_driver shift CRC NBYTES            crc32_shift(CRC, NBYTES)
//   crc32_driver parts FILE LEN...           the XOR of crc32_shift(crc(part), bytes behind it) over the parts
#include "crc32_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace hcamd::crc32;

static constexpr Tables kT = make_tables();
static constexpr ShiftTable kS = make_shift_table();
static_assert(kT.t[0][1] == 0x77073096u, "byte table");
static_assert(kS.x2n[0] == 0x00800000u, "x^8");

static std::vector<uint8_t> read_file(const char* path)
{
  std::vector<uint8_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f)
    std::exit(2);
  int c;
  while ((c = std::fgetc(f)) != EOF)
    v.push_back((uint8_t)c);
  std::fclose(f);
  return v;
}

static uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// slice-by-16 over p[0, n), the first `lead` bytes one at a time
static uint32_t crc_sliced(const uint8_t* p, size_t n, size_t lead)
{
  lead = lead < n ? lead : n;
  uint32_t reg = crc32_update_bytes(kT.t[0], 0xFFFFFFFFu, p, lead);
  size_t i = lead;
  for (; i + 16 <= n; i += 16)
    reg = crc32_update_16(kT, reg, le32(p + i), le32(p + i + 4), le32(p + i + 8), le32(p + i + 12));
  reg = crc32_update_bytes(kT.t[0], reg, p + i, n - i);
  return ~reg;
}

int main(int argc, char** argv)
{
  if (argc < 2)
    return 2;
  const std::string cmd = argv[1];
  if (cmd == "tables") {
    for (int k = 0; k < kSlices; ++k)
      for (int b = 0; b < 256; ++b)
        std::printf("%08x%c", kT.t[k][b], b == 255 ? '\n' : ' ');
  } else if (cmd == "crc" && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    std::printf("%u", crc32_of(kT, d.data(), d.size()));
    for (size_t lead = 0; lead < 16; ++lead)
      std::printf(" %u", crc_sliced(d.data(), d.size(), lead));
    std::printf("\n");
  } else if (cmd == "shift" && argc == 4) {
    std::printf("%u\n", crc32_shift(kS.x2n, (uint32_t)std::strtoul(argv[2], nullptr, 0), std::strtoull(argv[3], nullptr, 0)));
  } else if (cmd == "parts" && argc >= 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    uint64_t at = 0, total = 0;
    for (int k = 3; k < argc; ++k)
      total += std::strtoull(argv[k], nullptr, 0);
    if (total != d.size())
      return 3;
    uint32_t full = 0;
    for (int k = 3; k < argc; ++k) {
      const uint64_t len = std::strtoull(argv[k], nullptr, 0);
      full ^= crc32_shift(kS.x2n, crc32_of(kT, d.data() + at, len), total - at - len);
      at += len;
    }
    std::printf("%u\n", full);
  } else {
    return 2;
  }
  return 0;
}
