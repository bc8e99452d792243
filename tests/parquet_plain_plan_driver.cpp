// parquet_plain_plan_driver.cpp -- prints what hipcomp-core_amd/csrc/parquet_plain_plan.hpp makes of a list of items, for
// tests/test_parquet_plain_plan_cpu.py: a program of its own, compiled with g++ alone (no HIP) under the address and
// undefined-behaviour sanitizers.  Every array of an item is a heap buffer of exactly its length and every output one of
// exactly its capacity, so a read or a write outside either is the sanitizer's to report.
//
//   parquet_plain_plan_driver POOL LIST OUT
// LIST: a line per item, places and lengths in POOL (tests/parquet_plaingen.py, Item.line, writes them):
//   V src length start num_values has_levels levels rows max_level capacity value_bytes layout
//   B src length start num_values has_levels levels rows max_level capacity
//   S src length start num_values has_levels levels rows max_level offsets count offset_capacity byte_capacity layout
// Per item a line "item k status s count c"; OUT gets every output of every item, the whole capacity, back to back:
// the values and the bitmap (V); the bits and the bitmap (B); the offsets, the bytes and the bitmap (S).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "parquet_plain_plan.hpp"

using namespace hcamd::pqv;

// the header's functions are constexpr in earnest: items worked by the compiler
constexpr uint32_t placed(uint32_t layout)
{
  // three values of 2 bytes, 0x0201 0x0403 0x0605, behind a start of 1; five rows, the second and the fourth null
  const uint8_t plain[] = {9, 1, 2, 3, 4, 5, 6}, split_up[] = {9, 1, 3, 5, 2, 4, 6};
  const uint8_t levels[] = {1, 0, 1, 0, 1};
  uint8_t out[10] = {9, 9, 9, 9, 9, 9, 9, 9, 9, 9}, validity[1] = {0xFF};
  const Rows r = rows_of(3, levels, 5, 1);
  return place_values_item(layout == kPlain ? plain : split_up, 7, 1, r, 5, 2, layout, out, validity) && out[0] == 1 && out[1] == 2 && out[2] == 0
                 && out[3] == 0 && out[4] == 3 && out[5] == 4 && out[6] == 0 && out[7] == 0 && out[8] == 5 && out[9] == 6
             ? validity[0]
             : 0xFFu;
}
static_assert(placed(kPlain) == 21 && placed(kByteStreamSplit) == 21, "place_values_item");
constexpr uint32_t placed_bits()
{
  const uint8_t src[] = {0x05}, levels[] = {1, 0, 1, 1}; // true false true
  uint8_t out[1] = {0xFF}, validity[1] = {0xFF};
  const Rows r = rows_of(3, levels, 4, 1);
  return place_booleans_item(src, 1, 0, r, 4, out, validity) && validity[0] == 13 ? out[0] : 0xFFu;
}
static_assert(placed_bits() == 9, "place_booleans_item");
constexpr int64_t placed_strings(uint32_t layout)
{
  const uint8_t prefixed[] = {2, 0, 0, 0, 'a', 'b', 0, 0, 0, 0, 1, 0, 0, 0, 'c'}, packed[] = {'a', 'b', 'c'};
  const int32_t offsets[] = {0, 2, 2, 3};
  const uint8_t levels[] = {1, 1, 0, 1};
  int32_t out[5] = {-1, -1, -1, -1, -1};
  uint8_t bytes[3] = {0, 0, 0};
  const Rows r = rows_of(3, levels, 4, 1);
  const Strings v = layout == kLengthPrefixed ? place_strings_item(prefixed, 15, 0, offsets, r, layout, 5, 3, out, bytes, nullptr)
                                              : place_strings_item(packed, 3, 0, offsets, r, layout, 5, 3, out, bytes, nullptr);
  return v.ok && out[0] == 0 && out[1] == 2 && out[2] == 2 && out[3] == 2 && out[4] == 3 && bytes[0] == 'a' && bytes[1] == 'b' && bytes[2] == 'c'
             ? (int64_t)v.bytes
             : -1;
}
static_assert(placed_strings(kLengthPrefixed) == 3 && placed_strings(kPacked) == 3, "place_strings_item");
static_assert(start_refused(5, 4) && !start_refused(4, 4) && values_fit(3, 5, 15) && !values_fit(3, 5, 14), "the source");
static_assert(bits_fit(8, 1) && !bits_fit(9, 1) && bits_fit(0, 0) && !bits_fit(~uint64_t(0), 100), "bits_fit");
static_assert(string_refused(kPacked, 0, 0, 4, 3) && !string_refused(kPacked, 0, 0, 3, 3) && string_refused(kLengthPrefixed, 0, 0, 3, 6)
                  && !string_refused(kLengthPrefixed, 0, 0, 3, 7) && string_refused(kPacked, 2, 3, 2, 100) && string_refused(kPacked, 2, -1, 2, 100),
              "string_refused");
static_assert(value_byte_at(kPlain, 3, 1, 4, 10) == 13 && value_byte_at(kByteStreamSplit, 3, 1, 4, 10) == 13
                  && value_byte_at(kByteStreamSplit, 3, 2, 4, 10) == 23,
              "value_byte_at");

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
    uint64_t src_at, src_bytes, start, num_values, has_levels, lvl_at, rows, max_level;
    if (!(ls >> kind >> src_at >> src_bytes >> start >> num_values >> has_levels >> lvl_at >> rows >> max_level)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    const Exact<uint8_t> src(pool, src_at, src_bytes);
    const Exact<uint8_t> levels(pool, lvl_at, has_levels ? rows : 0);
    const Rows r = rows_of(num_values, has_levels ? levels.p : nullptr, rows, (uint32_t)max_level);
    Output<uint8_t> validity(bitmap_bytes(rows));
    bool ok = false;
    uint64_t count = 0;
    if (kind == "V") {
      uint64_t capacity, value_bytes, layout;
      if (!(ls >> capacity >> value_bytes >> layout))
        return 2;
      Output<uint8_t> values(capacity * value_bytes);
      ok = place_values_item(src.p, src_bytes, start, r, capacity, (uint32_t)value_bytes, (uint32_t)layout, values.p, validity.p);
      values.write(out);
    } else if (kind == "B") {
      uint64_t capacity;
      if (!(ls >> capacity))
        return 2;
      Output<uint8_t> bits(bitmap_bytes(capacity));
      ok = place_booleans_item(src.p, src_bytes, start, r, capacity, bits.p, validity.p);
      bits.write(out);
    } else {
      uint64_t off_at, off_count, offset_capacity, byte_capacity, layout;
      if (kind != "S" || !(ls >> off_at >> off_count >> offset_capacity >> byte_capacity >> layout))
        return 2;
      const Exact<int32_t> offsets(pool, off_at, off_count);
      Output<int32_t> off(offset_capacity);
      Output<uint8_t> bytes(byte_capacity);
      const Strings v = place_strings_item(src.p, src_bytes, start, offsets.p, r, (uint32_t)layout, offset_capacity, byte_capacity, off.p,
                                           bytes.p, validity.p);
      ok = v.ok;
      count = v.bytes;
      off.write(out);
      bytes.write(out);
    }
    validity.write(out);
    std::printf("item %zu status %d count %llu\n", k, ok ? 0 : 12, (unsigned long long)count);
    ++k;
  }
  return 0;
}
