// CPU driver of hipcomp-core_amd/csrc/deflate/deflate_tables.hpp (tests/test_deflate_tables_cpu.py): g++, standard
// headers, no HIP.  One case per line on stdin:
//   set <kind 0|1|2> <n> <n lengths>   -> "verdict <name>": the verdict on one set of code lengths
//                                         (0 code-length, 1 literal/length, 2 distance alphabet)
//   block <hex bytes>                  -> the first block of a raw Deflate stream, fixed or dynamic, decoded with
//                                         the header's tables and lookups alone:
//                                         "ok <symbols>" (L<byte>, M<length>,<distance>, up to the end-of-block
//                                         code) or "reject <verdict name>"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "deflate/deflate_tables.hpp"

using namespace hcamd::deflate;

namespace {

struct Bits
{
  const std::vector<uint8_t>& data;
  uint64_t pos = 0; // in bits
  bool over = false;
  uint32_t peek(int n)
  {
    uint32_t v = 0;
    for (int k = 0; k < n; ++k) {
      const uint64_t p = pos + (uint64_t)k;
      if (p / 8 < data.size())
        v |= (uint32_t)((data[p / 8] >> (p % 8)) & 1u) << k;
    }
    return v;
  }
  void drop(int n)
  {
    pos += (uint64_t)n;
    over = over || pos > 8 * (uint64_t)data.size();
  }
  uint32_t take(int n)
  {
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
};

Table<kFixedLitLen, kLitFastBits> lit;
Table<kFixedDist, kDistFastBits> dist;
Table<kNumCodeLen, kCodeLenFastBits> cl;

Verdict decode_block(const std::vector<uint8_t>& bytes, std::string& symbols)
{
  Bits in{bytes};
  in.take(1);
  const uint32_t btype = in.take(2);
  uint8_t lengths[kFixedLitLen + kFixedDist] = {};
  uint32_t hlit = kFixedLitLen, hdist = kFixedDist;
  if (btype == 1) {
    for (uint32_t i = 0; i < (uint32_t)kFixedLitLen; ++i)
      lengths[i] = (uint8_t)fixed_litlen_length(i);
    for (uint32_t i = 0; i < (uint32_t)kFixedDist; ++i)
      lengths[kFixedLitLen + i] = (uint8_t)kFixedDistLength;
  } else if (btype == 2) {
    hlit = in.take(5) + 257;
    hdist = in.take(5) + 1;
    const uint32_t hclen = in.take(4) + 4;
    if (verdict_header(hlit, hdist) != kOk)
      return verdict_header(hlit, hdist);
    uint8_t cll[kNumCodeLen] = {};
    for (uint32_t i = 0; i < hclen; ++i)
      cll[kCodeLenOrder[i]] = (uint8_t)in.take(3);
    if (in.over)
      return kTruncated;
    const Verdict vc = build_table(cll, kNumCodeLen, kCodeLen, cl);
    if (vc != kOk)
      return vc;
    uint32_t have = 0, prev = 0;
    while (have < hlit + hdist) {
      const uint32_t e = lookup(cl, in.peek(15));
      if (e == 0)
        return kBadSymbol;
      in.drop((int)(e & 15u));
      const uint32_t sym = e >> 4, extra = in.take((int)code_len_extra_bits(sym));
      if (in.over)
        return kTruncated;
      uint32_t value = 0, count = 0;
      const Verdict vr = code_len_run(sym, extra, have, hlit + hdist, prev, value, count);
      if (vr != kOk)
        return vr;
      for (uint32_t j = 0; j < count; ++j)
        lengths[have + j] = (uint8_t)value;
      have += count;
      prev = value;
    }
  } else {
    return kBadSymbol;
  }
  const Verdict vl = build_table(lengths, (int)hlit, kLitLen, lit);
  if (vl != kOk)
    return vl;
  const Verdict vd = build_table(lengths + hlit, (int)hdist, kDist, dist);
  if (vd != kOk)
    return vd;
  for (;;) {
    const uint32_t e = lookup(lit, in.peek(15));
    if (e == 0)
      return kBadSymbol;
    in.drop((int)(e & 15u));
    const uint32_t sym = e >> 4;
    if (in.over)
      return kTruncated;
    if (sym < 256) {
      symbols += " L" + std::to_string(sym);
      continue;
    }
    if (sym == (uint32_t)kEndOfBlock)
      return kOk;
    if (sym >= (uint32_t)kMaxLitLen)
      return kBadSymbol;
    const uint32_t length = kLengthBase[sym - 257] + in.take(kLengthExtra[sym - 257]);
    const uint32_t de = lookup(dist, in.peek(15));
    if (de == 0)
      return kBadSymbol;
    in.drop((int)(de & 15u));
    const uint32_t ds = de >> 4;
    if (ds >= (uint32_t)kMaxDist)
      return kBadSymbol;
    const uint32_t distance = kDistBase[ds] + in.take(kDistExtra[ds]);
    if (in.over)
      return kTruncated;
    symbols += " M" + std::to_string(length) + "," + std::to_string(distance);
  }
}

} // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string what;
    is >> what;
    if (what == "set") {
      int kind = 0, n = 0;
      is >> kind >> n;
      std::vector<uint8_t> lengths((size_t)n);
      for (int i = 0; i < n; ++i) {
        int v = 0;
        is >> v;
        lengths[(size_t)i] = (uint8_t)v;
      }
      Verdict v;
      if (kind == kCodeLen)
        v = build_table(lengths.data(), n, kCodeLen, cl);
      else if (kind == kLitLen)
        v = build_table(lengths.data(), n, kLitLen, lit);
      else
        v = build_table(lengths.data(), n, kDist, dist);
      std::printf("verdict %s\n", verdict_name(v));
    } else if (what == "block") {
      std::string hex;
      is >> hex;
      std::vector<uint8_t> bytes;
      for (size_t i = 0; i + 1 < hex.size(); i += 2)
        bytes.push_back((uint8_t)std::stoi(hex.substr(i, 2), nullptr, 16));
      std::string symbols;
      const Verdict v = decode_block(bytes, symbols);
      if (v == kOk)
        std::printf("ok%s\n", symbols.c_str());
      else
        std::printf("reject %s\n", verdict_name(v));
    } else if (!what.empty()) {
      std::fprintf(stderr, "unknown case '%s'\n", what.c_str());
      return 2;
    }
  }
  return 0;
}
