// parquet_dict_plan_driver.cpp -- prints what hipcomp-core_amd/csrc/parquet_dict_plan.hpp makes of a list of items, for
// tests/test_parquet_dict_plan_cpu.py: a program of its own, compiled with g++ alone (no HIP) under the address and
// undefined-behaviour sanitizers.  Every array of an item is a heap buffer of exactly its length and every output one of
// exactly its capacity, so a read or a write outside either is the sanitizer's to report.
//
//   parquet_dict_plan_driver POOL LIST OUT
// LIST: a line per item, places and lengths in POOL (tests/parquet_dictgen.py, Item.line, writes them):
//   I dict length entries capacity
//   F dict length dict_entries indices num_indices has_levels levels rows max_level capacity entry_bytes
//   S dict length dict_entries dict_offsets count indices num_indices has_levels levels rows max_level offset_capacity byte_capacity
// Per item a line "item k status s count c"; OUT gets every output of every item, the whole capacity, back to back:
// the offsets (I); the entries and the bitmap (F); the offsets, the bytes and the bitmap (S).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "parquet_dict_plan.hpp"

using namespace hcamd::pqg;

// the header's functions are constexpr in earnest: items worked by the compiler
constexpr int32_t third_offset()
{
  const uint8_t body[] = {2, 0, 0, 0, 'a', 'b', 0, 0, 0, 0, 3, 0, 0, 0, 'c', 'd', 'e', 9};
  int32_t off[4] = {-1, -1, -1, -1};
  return index_item(body, sizeof(body), 3, 4, off) && off[0] == 0 && off[1] == 2 && off[2] == 2 ? off[3] : -1;
}
static_assert(third_offset() == 5, "index_item");
constexpr uint32_t gathered()
{
  const uint8_t dict[] = {1, 2, 3, 4, 5, 6};
  const uint32_t indices[] = {2, 0};
  const uint8_t levels[] = {1, 0, 1};
  uint8_t out[6] = {9, 9, 9, 9, 9, 9}, validity[1] = {0xFF};
  const Rows r{indices, 2, levels, 3, 1};
  return gather_item(dict, 6, 3, r, 3, 2, out, validity) && out[0] == 5 && out[1] == 6 && out[2] == 0 && out[3] == 0 && out[4] == 1
                 && out[5] == 2
             ? validity[0]
             : 0xFFu;
}
static_assert(gathered() == 5, "gather_item");
static_assert(entry_refused(0, 0, 1, 4) && !entry_refused(0, 0, 1, 5) && entry_refused(1, 3, 2, 100) && entry_refused(1, -1, 2, 100),
              "entry_refused");
static_assert(output_alignment(12) == 4 && output_alignment(5) == 1 && output_alignment(64) == 8 && output_alignment(6) == 2, "alignment");
static_assert(!shape_of(true, 0, 5, 5, 1).ok && shape_of(true, 0, 5, 6, 1).ok && shape_of(false, 7, 99, 7, 0).rows == 7, "shape_of");

static const uint8_t kFill = 0xA5;

// a heap copy of exactly `count` elements of T from the pool
template <class T>
struct Exact
{
  T* p;
  Exact(const std::vector<uint8_t>& pool, uint64_t at, uint64_t count) : p(new T[count])
  {
    if (at + count * sizeof(T) > pool.size()) {
      std::fprintf(stderr, "an array lies outside the pool\n");
      std::exit(2);
    }
    if (count)
      std::memcpy(p, pool.data() + at, count * sizeof(T));
  }
  ~Exact() { delete[] p; }
};
// an output of exactly `count` elements, filled
template <class T>
struct Output
{
  T* p;
  uint64_t bytes;
  explicit Output(uint64_t count) : p(new T[count]), bytes(count * sizeof(T)) { std::memset(p, kFill, bytes); }
  ~Output() { delete[] p; }
  void write(std::ofstream& out) const { out.write(reinterpret_cast<const char*>(p), (std::streamsize)bytes); }
};

int main(int argc, char** argv)
{
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s POOL LIST OUT\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  const std::vector<uint8_t> pool((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::ifstream list(argv[2]);
  std::ofstream out(argv[3], std::ios::binary);
  std::string line;
  size_t k = 0;
  while (std::getline(list, line)) {
    std::istringstream ls(line);
    std::string kind;
    uint64_t dict_at, dict_bytes, entries;
    if (!(ls >> kind >> dict_at >> dict_bytes >> entries)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    const Exact<uint8_t> dict(pool, dict_at, dict_bytes);
    bool ok = false;
    uint64_t count = 0;
    if (kind == "I") {
      uint64_t capacity;
      if (!(ls >> capacity))
        return 2;
      Output<int32_t> off(capacity);
      ok = index_item(dict.p, dict_bytes, entries, capacity, off.p);
      count = ok ? entries : 0;
      off.write(out);
    } else {
      uint64_t doff_at = 0, doff_count = 0, idx_at, num_indices, has_levels, lvl_at, rows, max_level, cap_a, cap_b;
      if (kind == "S" && !(ls >> doff_at >> doff_count))
        return 2;
      if (!(ls >> idx_at >> num_indices >> has_levels >> lvl_at >> rows >> max_level >> cap_a >> cap_b))
        return 2;
      const Exact<uint32_t> indices(pool, idx_at, num_indices);
      const Exact<uint8_t> levels(pool, lvl_at, has_levels ? rows : 0);
      const Rows r{indices.p, num_indices, has_levels ? levels.p : nullptr, rows, (uint32_t)max_level};
      Output<uint8_t> validity(bitmap_bytes(rows));
      if (kind == "F") {
        Output<uint8_t> values(cap_a * cap_b);
        ok = gather_item(dict.p, dict_bytes, entries, r, cap_a, (uint32_t)cap_b, values.p, validity.p);
        values.write(out);
      } else {
        const Exact<int32_t> doff(pool, doff_at, doff_count);
        Output<int32_t> off(cap_a);
        Output<uint8_t> bytes(cap_b);
        const Strings v = gather_strings_item(dict.p, dict_bytes, entries, doff.p, r, cap_a, cap_b, off.p, bytes.p, validity.p);
        ok = v.ok;
        count = v.bytes;
        off.write(out);
        bytes.write(out);
      }
      validity.write(out);
    }
    std::printf("item %zu status %d count %llu\n", k, ok ? 0 : 12, (unsigned long long)count);
    ++k;
  }
  return 0;
}
