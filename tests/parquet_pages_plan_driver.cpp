// Prints what hipcomp-core_amd/csrc/parquet_pages_plan.hpp computes, for tests/test_parquet_pages_plan_cpu.py.  No HIP:
// g++ alone, under the address and undefined-behaviour sanitizers.
//   walk LIST            LIST: lines "FILE OFFSET LENGTH CODEC"; per item "item I ok K pages N out S bare B largest L
//                        fate_small F", then a line "page ..." per listed page: the fields of the record in order.
//                        Every item is copied into a buffer of exactly its length, so that a read outside it is seen.
//                        fate_small: fate_of with a table of one row less and an output of one byte less than needed
//   relist LIST MOST     the same pages from listing walks of at most MOST pages each, taken up where the last stopped
//   layout ITEMS P ROOM MOST
//   passes P COUNT...
#include "parquet_pages_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace hcamd::pqp;

namespace {

struct Bytes
{
  const uint8_t* p;
  uint64_t n;
  uint32_t at(uint64_t pos) const
  {
    if (pos >= n) { // (the plan promises never to ask)
      std::fprintf(stderr, "read at %" PRIu64 " of %" PRIu64 "\n", pos, n);
      std::abort();
    }
    return p[pos];
  }
};

struct Print
{
  void page(uint64_t, const Page& p)
  {
    std::printf("page %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u %u %u %u %u %u %u %u\n", p.header_offset, p.body_offset,
                p.out_offset, p.compressed_page_size, p.uncompressed_page_size, p.kind, p.num_values, p.encoding, p.rep_levels_bytes,
                p.def_levels_bytes, p.num_nulls, p.num_rows, p.crc, p.flags);
  }
};

std::vector<uint8_t> slice_of(const std::string& file, uint64_t offset, uint64_t length)
{
  std::ifstream f(file, std::ios::binary);
  if (!f)
    std::exit(3);
  f.seekg((std::streamoff)offset);
  std::vector<uint8_t> v(length);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)length);
  if ((uint64_t)f.gcount() != length)
    std::exit(3);
  return v;
}

int walk_list(const char* list, uint64_t most)
{
  std::ifstream f(list);
  std::string line;
  uint64_t item = 0;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string file;
    uint64_t offset = 0, length = 0;
    uint32_t codec = 0;
    in >> file >> offset >> length >> codec;
    const std::vector<uint8_t> held = slice_of(file, offset, length);
    // (a vector of no bytes may have no buffer at all: the plan is not to look)
    Bytes src{held.empty() ? nullptr : held.data(), length};
    NoSink none;
    const Walk w = walk_pages(src, length, codec, Walk(), ~uint64_t(0), none);
    const uint32_t small = fate_of(w, true, w.pages ? w.pages - 1 : 0, w.out ? w.out - 1 : 0);
    std::printf("item %" PRIu64 " ok %u pages %" PRIu64 " out %" PRIu64 " bare %u largest %" PRIu64 " fate_small %u\n", item, w.ok,
                w.ok ? w.pages : 0, w.ok ? w.out : 0, w.bare, w.largest, small);
    if (w.ok) {
      Print print;
      Walk at;
      uint64_t walks = 0;
      while (at.pages < w.pages) {
        at = walk_pages(src, length, codec, at, most, print);
        if (!at.ok || ++walks > w.pages)
          return 4;
      }
      if (at.out != w.out)
        return 4;
    }
    ++item;
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  static_assert(sizeof(Page) == 72, "the page record");
  if (argc < 2)
    return 2;
  const std::string mode = argv[1];
  auto num = [&](int i) { return (uint64_t)std::strtoull(argv[i], nullptr, 10); };
  if (mode == "walk" && argc == 3)
    return walk_list(argv[2], ~uint64_t(0));
  if (mode == "relist" && argc == 4)
    return walk_list(argv[2], num(3));
  if (mode == "layout" && argc == 6) {
    const uint64_t items = num(2), P = num(3), room = num(4), most = num(5);
    std::printf("items_bytes %" PRIu64 " totals_at %" PRIu64 " lists_at %" PRIu64 " scratch_bytes %" PRIu64
                " min_scratch_bytes %" PRIu64 " pass_entries %" PRIu64 " entry_bytes %" PRIu64,
                items_bytes(items), totals_at(items), lists_at(items), scratch_bytes(items, P), min_scratch_bytes(items),
                pass_entries(room, items, most), kEntryBytes);
    for (uint64_t j = 0; j < kLists8; ++j)
      std::printf(" list8_%" PRIu64 " %" PRIu64, j, list8_at(items, P, j));
    for (uint64_t j = 0; j < kLists4; ++j)
      std::printf(" list4_%" PRIu64 " %" PRIu64, j, list4_at(items, P, j));
    std::printf("\n");
    return 0;
  }
  if (mode == "passes" && argc >= 3) {
    const uint64_t P = num(2);
    std::vector<uint64_t> counts, first;
    uint64_t total = 0;
    for (int i = 3; i < argc; ++i) {
      first.push_back(total);
      counts.push_back(num(i));
      total += counts.back();
    }
    std::printf("total %" PRIu64 " passes %" PRIu64 "\n", total, passes_of(total, P));
    for (uint64_t k = 0; k < passes_of(total, P); ++k) {
      std::printf("pass %" PRIu64 " count %" PRIu64 "\n", k, pass_count(total, P, k));
      for (size_t i = 0; i < counts.size(); ++i) {
        const Slice s = item_slice(first[i], counts[i], P, k);
        if (s.count)
          std::printf("pass %" PRIu64 " item %zu at %" PRIu64 " count %" PRIu64 "\n", k, i, s.at, s.count);
      }
    }
    return 0;
  }
  return 2;
}
