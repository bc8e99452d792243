// parquet_plain_driver.cpp -- the three calls that put a Parquet page's dense values into their rows (hipcomp/cascaded.hpp:
// place_parquet_values, place_parquet_booleans, place_parquet_strings), driven for tests/test_parquet_plain_gpu.py: a C++
// program written against include/ and linked to libhipcomp.so.
//
//   parquet_plain_driver batch POOL LIST
// LIST: "case KIND value_bytes layout has_levels align nulls ones OUT items", then a line per item as
// tests/parquet_plaingen.py's Item.line writes it (places and lengths in POOL).  A case is one call.  Every output has 32
// guard bytes on both sides; with `align`, sources, validity arrays, values bitmaps and string bytes lie that many bytes
// behind an aligned address and the other outputs at the alignment the contract states, no better.  nulls: 1 without the
// count array, 2 without the validity array, 4 without device_value_starts (every item's start is 0 then).  ones: every
// item is also worked in a call of its own, into outputs of its own, and compared.  Per item "item k status s count c
// guards g (c: -1 where the call has no count array) [one_status s one_count c eq_one e]", then "case n"; OUT gets every
// output of every item, the whole capacity, back to back.
//
//   parquet_plain_driver chain POOL LIST OUT form KIND value_bytes layout
// LIST: a line per page, "page length levels_length rows cut": the page's level stream with its values section right
// behind.  The levels (form: decode_parquet_hybrid's) with the count of the ones; then
//   V, B         the place call, those counts as its device_num_values; a V1 page (form 1) is handed over whole, the
//                levels' consumed bytes as device_value_starts; a V2 page's values section with no starts
//   D            decode_parquet_delta(Values, LONGLONG) of the values section, then place_parquet_values of 8 bytes
//                with the delta call's value counts
//   S layout 0   index_parquet_dictionary of the values section less `cut` bytes, then place_parquet_strings with the
//                index call's entry counts
//   S layout 1   decode_parquet_delta(Offsets, INT) of the same, then place_parquet_strings with its value counts and
//                its consumed bytes as device_value_starts
// nothing is read back and nothing waits between the calls.  OUT: per page the levels, then the outputs as above.
//
//   parquet_plain_driver misuse
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "hipcomp/cascaded.hpp"
#ifdef PLAIN_HOST_PATH
#include <algorithm>

#include "parquet_plain_plan.hpp" // the host path of `time`: what a user without the calls runs
#endif

#define HIP_OK(x)                                                                                  \
  do {                                                                                             \
    const hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) {                                                                        \
      std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
      std::exit(3);                                                                                \
    }                                                                                              \
  } while (0)

static const uint8_t kFill = 0xA5, kGuard = 0x5A;
static const size_t kGuardBytes = 32;

static std::vector<uint8_t> read_file(const char* path)
{
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a host image of a device buffer, pieces placed at 16-byte addresses plus `behind`
struct Arena
{
  std::vector<uint8_t> host;
  uint8_t* dev = nullptr;
  std::map<std::pair<uint64_t, uint64_t>, size_t> shared; // the sources put so far: (place in the pool, bytes) -> place here
  size_t place(size_t bytes, size_t behind, bool guarded)
  {
    size_t at = host.size() + (guarded ? kGuardBytes : 0);
    at = (at + 15) / 16 * 16 + behind;
    host.resize(at, kGuard);
    host.resize(at + bytes, kFill);
    host.resize(at + bytes + (guarded ? kGuardBytes : 0), kGuard);
    return at;
  }
  size_t put(const std::vector<uint8_t>& pool, size_t from, size_t bytes, size_t behind)
  {
    if (from + bytes > pool.size()) {
      std::fprintf(stderr, "an array lies outside the pool\n");
      std::exit(2);
    }
    const size_t at = place(bytes, behind, false);
    if (bytes)
      std::memcpy(host.data() + at, pool.data() + from, bytes);
    return at;
  }
  void upload()
  {
    HIP_OK(hipMalloc(&dev, host.size() + 16));
    HIP_OK(hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice));
  }
  void download(std::vector<uint8_t>& to) const
  {
    to.resize(host.size());
    HIP_OK(hipMemcpy(to.data(), dev, host.size(), hipMemcpyDeviceToHost));
  }
  ~Arena()
  {
    if (dev)
      (void)hipFree(dev);
  }
};

template <class T>
struct DeviceArray
{
  T* p = nullptr;
  size_t n = 0;
  DeviceArray() {}
  explicit DeviceArray(const std::vector<T>& v) : n(v.size())
  {
    HIP_OK(hipMalloc(&p, (n + 1) * sizeof(T)));
    if (n)
      HIP_OK(hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  DeviceArray(size_t count, int byte) : n(count)
  {
    HIP_OK(hipMalloc(&p, (n + 1) * sizeof(T)));
    HIP_OK(hipMemset(p, byte, (n + 1) * sizeof(T)));
  }
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  std::vector<T> get() const
  {
    std::vector<T> v(n);
    if (n)
      HIP_OK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
  }
  ~DeviceArray()
  {
    if (p)
      (void)hipFree(p);
  }
};

// an item as its line has it, and where its arrays and outputs lie in the arenas
struct Item
{
  char kind = 'V';
  uint64_t src_at = 0, src_bytes = 0, start = 0, num_values = 0, has_levels = 0, lvl_at = 0, rows = 0, max_level = 0, off_at = 0,
           off_count = 0, cap_a = 0, cap_b = 0, value_bytes = 0, layout = 0;
  size_t in_src = 0, in_lvl = 0, in_off = 0;
  size_t out[3] = {0, 0, 0}, out_bytes[3] = {0, 0, 0};
  int outs = 0;
};

static bool parse_item(const std::string& line, Item& it)
{
  std::istringstream ls(line);
  std::string kind;
  if (!(ls >> kind >> it.src_at >> it.src_bytes >> it.start >> it.num_values >> it.has_levels >> it.lvl_at >> it.rows >> it.max_level)
      || kind.size() != 1)
    return false;
  it.kind = kind[0];
  if (it.kind == 'V')
    return (bool)(ls >> it.cap_a >> it.value_bytes >> it.layout);
  if (it.kind == 'B')
    return (bool)(ls >> it.cap_a);
  return it.kind == 'S' && (bool)(ls >> it.off_at >> it.off_count >> it.cap_a >> it.cap_b >> it.layout);
}

// With `align`, an output lies at the alignment the contract states and no better: an odd multiple of it.
static size_t stated(size_t align, size_t element_bytes)
{
  size_t a = 1;
  while (a < 8 && element_bytes % (2 * a) == 0)
    a *= 2;
  return align ? a : 0;
}

static void lay_outputs(Item& it, Arena& out, size_t align)
{
  const size_t validity = (it.rows + 7) / 8;
  if (it.kind == 'V') {
    it.outs = 2;
    it.out_bytes[0] = it.cap_a * it.value_bytes;
    it.out[0] = out.place(it.out_bytes[0], stated(align, it.value_bytes), true);
  } else if (it.kind == 'B') {
    it.outs = 2;
    it.out_bytes[0] = (it.cap_a + 7) / 8;
    it.out[0] = out.place(it.out_bytes[0], align, true);
  } else {
    it.outs = 3;
    it.out_bytes[0] = 4 * it.cap_a;
    it.out[0] = out.place(it.out_bytes[0], stated(align, 4), true);
    it.out_bytes[1] = it.cap_b;
    it.out[1] = out.place(it.out_bytes[1], align, true);
  }
  it.out_bytes[it.outs - 1] = validity;
  it.out[it.outs - 1] = out.place(validity, align, true);
}

static void lay_out(Item& it, const std::vector<uint8_t>& pool, Arena& in, Arena& out, size_t align)
{
  // (items that name the same bytes of the pool share one source)
  const auto key = std::make_pair(it.src_at, it.src_bytes);
  if (!in.shared.count(key))
    in.shared[key] = in.put(pool, it.src_at, it.src_bytes, align);
  it.in_src = in.shared[key];
  it.in_lvl = in.put(pool, it.lvl_at, it.has_levels ? it.rows : 0, 0);
  if (it.kind == 'S')
    it.in_off = in.put(pool, it.off_at, 4 * it.off_count, 0);
  lay_outputs(it, out, align);
}

// the device arrays of a call over items [0, n), outputs in `out`
struct Call
{
  std::vector<const uint8_t*> src_ptrs, level_ptrs;
  std::vector<size_t> src_bytes, starts, num_values, rows, cap_a, cap_b;
  std::vector<const int32_t*> off_ptrs;
  std::vector<uint32_t> max_levels;
  std::vector<void*> out0;
  std::vector<uint8_t*> out1, validity;
  Call(const std::vector<Item>& items, const Arena& in, const Arena& out)
  {
    for (const Item& it : items) {
      src_ptrs.push_back(in.dev + it.in_src);
      src_bytes.push_back(it.src_bytes);
      starts.push_back(it.start);
      num_values.push_back(it.num_values);
      level_ptrs.push_back(in.dev + it.in_lvl);
      rows.push_back(it.rows);
      max_levels.push_back((uint32_t)it.max_level);
      off_ptrs.push_back(reinterpret_cast<const int32_t*>(in.dev + it.in_off));
      cap_a.push_back(it.cap_a);
      cap_b.push_back(it.cap_b);
      out0.push_back(out.dev + it.out[0]);
      out1.push_back(out.dev + it.out[1]);
      validity.push_back(out.dev + it.out[it.outs - 1]);
    }
  }
};

struct DeviceCall
{
  DeviceArray<const uint8_t*> src_ptrs, level_ptrs;
  DeviceArray<size_t> src_bytes, starts, num_values, rows, cap_a, cap_b;
  DeviceArray<const int32_t*> off_ptrs;
  DeviceArray<uint32_t> max_levels;
  DeviceArray<void*> out0;
  DeviceArray<uint8_t*> out1, validity;
  explicit DeviceCall(const Call& c)
      : src_ptrs(c.src_ptrs), level_ptrs(c.level_ptrs), src_bytes(c.src_bytes), starts(c.starts), num_values(c.num_values), rows(c.rows),
        cap_a(c.cap_a), cap_b(c.cap_b), off_ptrs(c.off_ptrs), max_levels(c.max_levels), out0(c.out0), out1(c.out1), validity(c.validity)
  {
  }
  // items [first, first + n) in one call
  void run(hipcomp::CascadedManager& m, char kind, uint32_t value_bytes, uint32_t layout, bool has_levels, int nulls, size_t first, size_t n,
           hipcompStatus_t* statuses, size_t* counts) const
  {
    size_t* const count = (nulls & 1) ? nullptr : counts + first;
    uint8_t* const* const valid = (nulls & 2) ? nullptr : validity.p + first;
    const size_t* const begin = (nulls & 4) ? nullptr : starts.p + first;
    const uint8_t* const* const levels = has_levels ? level_ptrs.p + first : nullptr;
    const size_t* const num_rows = has_levels ? rows.p + first : nullptr;
    const uint32_t* const maxima = has_levels ? max_levels.p + first : nullptr;
    if (kind == 'V')
      m.place_parquet_values(src_ptrs.p + first, src_bytes.p + first, begin, num_values.p + first, levels, num_rows, maxima, out0.p + first,
                             cap_a.p + first, valid, statuses + first, n, value_bytes, (hipcomp::ParquetValueLayout)layout);
    else if (kind == 'B')
      m.place_parquet_booleans(src_ptrs.p + first, src_bytes.p + first, begin, num_values.p + first, levels, num_rows, maxima,
                               reinterpret_cast<uint8_t* const*>(out0.p + first), cap_a.p + first, valid, statuses + first, n);
    else
      m.place_parquet_strings(src_ptrs.p + first, src_bytes.p + first, begin, off_ptrs.p + first, num_values.p + first, levels, num_rows,
                              maxima, reinterpret_cast<int32_t* const*>(out0.p + first), cap_a.p + first, out1.p + first, cap_b.p + first,
                              count, valid, statuses + first, n, (hipcomp::ParquetStringLayout)layout);
  }
};

// every byte of the arena that is no output of an item is a guard or an alignment gap: both hold kGuard
static bool guards_of(const Item& it, const std::vector<uint8_t>& got)
{
  bool ok = true;
  for (int o = 0; o < it.outs; ++o)
    for (size_t g = 0; g < kGuardBytes; ++g)
      ok = ok && got[it.out[o] - 1 - g] == kGuard && got[it.out[o] + it.out_bytes[o] + g] == kGuard;
  return ok;
}

static int batch(const char* pool_path, const char* list_path)
{
  const std::vector<uint8_t> pool = read_file(pool_path);
  std::ifstream list(list_path);
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  {
    hipcomp::CascadedManager manager(hipcompBatchedCascadedDefaultOpts, stream, 0);
    std::string line;
    while (std::getline(list, line)) {
      std::istringstream ls(line);
      std::string word, kind, out_path;
      uint32_t value_bytes, layout;
      int has_levels, nulls, ones;
      size_t align, n;
      if (!(ls >> word >> kind >> value_bytes >> layout >> has_levels >> align >> nulls >> ones >> out_path >> n) || word != "case") {
        std::fprintf(stderr, "bad case: %s\n", line.c_str());
        return 2;
      }
      std::vector<Item> items(n);
      Arena in, out, alone;
      for (size_t k = 0; k < n; ++k) {
        if (!std::getline(list, line) || !parse_item(line, items[k]) || items[k].kind != kind[0]) {
          std::fprintf(stderr, "bad item: %s\n", line.c_str());
          return 2;
        }
        if ((nulls & 4) && items[k].start != 0) {
          std::fprintf(stderr, "an item with a start in a case without starts: %s\n", line.c_str());
          return 2;
        }
        lay_out(items[k], pool, in, out, align);
      }
      alone.host = out.host;
      in.upload();
      out.upload();
      const uint8_t status_fill = 0x77;
      DeviceArray<hipcompStatus_t> statuses(n, status_fill), one_statuses(n, status_fill);
      DeviceArray<size_t> counts(n, status_fill), one_counts(n, status_fill);
      const DeviceCall call((Call(items, in, out)));
      call.run(manager, kind[0], value_bytes, layout, has_levels != 0, nulls, 0, n, statuses.p, counts.p);
      HIP_OK(hipStreamSynchronize(stream));
      std::vector<uint8_t> got, got_alone;
      out.download(got);
      if (ones) {
        alone.upload();
        const DeviceCall each((Call(items, in, alone)));
        for (size_t k = 0; k < n; ++k)
          each.run(manager, kind[0], value_bytes, layout, has_levels != 0, nulls, k, 1, one_statuses.p, one_counts.p);
        HIP_OK(hipStreamSynchronize(stream));
        alone.download(got_alone);
      }
      const std::vector<hipcompStatus_t> st = statuses.get(), one_st = one_statuses.get();
      const std::vector<size_t> ct = counts.get(), one_ct = one_counts.get();
      std::ofstream dump(out_path, std::ios::binary);
      const bool no_count = (nulls & 1) || kind[0] != 'S'; // (only the strings' call reports a count)
      for (size_t k = 0; k < n; ++k) {
        const Item& it = items[k];
        std::printf("item %zu status %d count %lld guards %d", k, (int)st[k], no_count ? -1ll : (long long)ct[k], (int)guards_of(it, got));
        if (ones) {
          bool same = guards_of(it, got_alone);
          for (int o = 0; o < it.outs; ++o)
            same = same && std::memcmp(got.data() + it.out[o], got_alone.data() + it.out[o], it.out_bytes[o]) == 0;
          std::printf(" one_status %d one_count %lld eq_one %d", (int)one_st[k], no_count ? -1ll : (long long)one_ct[k], (int)same);
        }
        std::printf("\n");
        for (int o = 0; o < it.outs; ++o)
          dump.write(reinterpret_cast<const char*>(got.data() + it.out[o]), (std::streamsize)it.out_bytes[o]);
      }
      std::printf("case %zu\n", n);
    }
  }
  HIP_OK(hipStreamDestroy(stream));
  return 0;
}

static int chain(const char* pool_path, const char* list_path, const char* out_path, int form, char kind, uint32_t value_bytes, uint32_t layout)
{
  const std::vector<uint8_t> pool = read_file(pool_path);
  std::ifstream list(list_path);
  std::string line;
  std::vector<Item> items;
  Arena in, out;
  const bool whole_page = form == 1 && (kind == 'V' || kind == 'B'); // a V1 page handed over whole, the start from the levels' call
  std::vector<size_t> in_page, lvl_len, values_len, out_levels, out_mid;
  while (std::getline(list, line)) {
    std::istringstream ls(line);
    uint64_t page_at, page_len, levels_len, cut;
    Item it;
    if (!(ls >> page_at >> page_len >> levels_len >> it.rows >> cut) || levels_len > page_len || cut > page_len - levels_len) {
      std::fprintf(stderr, "bad page: %s\n", line.c_str());
      return 2;
    }
    it.kind = kind == 'D' ? 'V' : kind;
    it.value_bytes = kind == 'D' ? 8 : value_bytes;
    it.layout = kind == 'D' ? 0 : layout;
    it.has_levels = 1;
    it.max_level = 1;
    it.cap_a = kind == 'S' ? it.rows + 1 : it.rows;
    it.cap_b = kind == 'S' ? 400 * it.rows : 0; // (no fixture string is longer)
    in_page.push_back(in.put(pool, page_at, page_len, 1));
    lvl_len.push_back(levels_len);
    values_len.push_back(page_len - levels_len - cut);
    lay_outputs(it, out, 1);
    // what the earlier calls write: outputs too, but of this program's own
    out_levels.push_back(out.place(it.rows, 0, true));
    out_mid.push_back(out.place(8 * (it.rows + 1), 0, true)); // the delta call's values, or either call's offsets
    items.push_back(it);
  }
  const size_t n = items.size();
  in.upload();
  out.upload();
  Call c(items, in, out);
  std::vector<const uint8_t*> lvl_streams, value_ptrs;
  std::vector<size_t> lvl_bytes, mid_caps, dense_bytes;
  std::vector<void*> lvl_outs, mid_outs;
  for (size_t k = 0; k < n; ++k) {
    lvl_streams.push_back(in.dev + in_page[k]);
    lvl_bytes.push_back(form == 1 ? lvl_len[k] + values_len[k] : lvl_len[k]);
    value_ptrs.push_back(in.dev + in_page[k] + lvl_len[k]);
    lvl_outs.push_back(out.dev + out_levels[k]);
    mid_outs.push_back(out.dev + out_mid[k]);
    mid_caps.push_back(kind == 'S' ? items[k].rows + 1 : items[k].rows);
    dense_bytes.push_back(8 * items[k].rows);
    c.level_ptrs[k] = out.dev + out_levels[k];
    c.off_ptrs[k] = reinterpret_cast<const int32_t*>(out.dev + out_mid[k]);
    if (whole_page) {
      c.src_ptrs[k] = lvl_streams[k];
      c.src_bytes[k] = lvl_bytes[k];
    } else if (kind == 'D') {
      c.src_ptrs[k] = out.dev + out_mid[k];
      c.src_bytes[k] = dense_bytes[k];
    } else {
      c.src_ptrs[k] = value_ptrs[k];
      c.src_bytes[k] = values_len[k];
    }
  }
  const DeviceCall call(c);
  const DeviceArray<const uint8_t*> d_lvl_streams(lvl_streams), d_value_ptrs(value_ptrs);
  const DeviceArray<void*> d_lvl_outs(lvl_outs), d_mid_outs(mid_outs);
  const DeviceArray<size_t> d_lvl_bytes(lvl_bytes), d_values_len(values_len), d_mid_caps(mid_caps);
  const DeviceArray<uint32_t> ones(std::vector<uint32_t>(n, 1u));
  const uint8_t fill = 0x77;
  DeviceArray<size_t> non_null(n, fill), consumed(n, fill), mid_counts(n, fill), mid_consumed(n, fill), byte_counts(n, fill);
  DeviceArray<hipcompStatus_t> lvl_status(n, fill), mid_status(n, fill), status(n, fill);
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  {
    hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
    // nothing is read back and nothing waits between these calls
    m.decode_parquet_hybrid(d_lvl_streams.p, d_lvl_bytes.p, ones.p, call.rows.p, d_lvl_outs.p, call.rows.p, consumed.p, ones.p, non_null.p,
                            lvl_status.p, n, (hipcomp::ParquetHybridForm)form, HIPCOMP_TYPE_UCHAR);
    if (kind == 'V')
      m.place_parquet_values(call.src_ptrs.p, call.src_bytes.p, whole_page ? consumed.p : nullptr, non_null.p, call.level_ptrs.p, call.rows.p,
                             call.max_levels.p, call.out0.p, call.cap_a.p, call.validity.p, status.p, n, value_bytes,
                             (hipcomp::ParquetValueLayout)layout);
    else if (kind == 'B')
      m.place_parquet_booleans(call.src_ptrs.p, call.src_bytes.p, whole_page ? consumed.p : nullptr, non_null.p, call.level_ptrs.p, call.rows.p,
                               call.max_levels.p, reinterpret_cast<uint8_t* const*>(call.out0.p), call.cap_a.p, call.validity.p, status.p, n);
    else if (kind == 'D') {
      m.decode_parquet_delta(d_value_ptrs.p, d_values_len.p, non_null.p, d_mid_outs.p, d_mid_caps.p, mid_counts.p, nullptr, mid_status.p, n,
                             hipcomp::ParquetDeltaOutput::Values, HIPCOMP_TYPE_LONGLONG);
      m.place_parquet_values(call.src_ptrs.p, call.src_bytes.p, nullptr, mid_counts.p, call.level_ptrs.p, call.rows.p, call.max_levels.p,
                             call.out0.p, call.cap_a.p, call.validity.p, status.p, n, 8, hipcomp::ParquetValueLayout::Plain);
    } else if (layout == 0) {
      m.index_parquet_dictionary(d_value_ptrs.p, d_values_len.p, non_null.p, reinterpret_cast<int32_t* const*>(d_mid_outs.p), d_mid_caps.p,
                                 mid_counts.p, mid_status.p, n);
      m.place_parquet_strings(call.src_ptrs.p, call.src_bytes.p, nullptr, call.off_ptrs.p, mid_counts.p, call.level_ptrs.p, call.rows.p,
                              call.max_levels.p, reinterpret_cast<int32_t* const*>(call.out0.p), call.cap_a.p, call.out1.p, call.cap_b.p,
                              byte_counts.p, call.validity.p, status.p, n, hipcomp::ParquetStringLayout::LengthPrefixed);
    } else {
      m.decode_parquet_delta(d_value_ptrs.p, d_values_len.p, non_null.p, d_mid_outs.p, d_mid_caps.p, mid_counts.p, mid_consumed.p, mid_status.p,
                             n, hipcomp::ParquetDeltaOutput::Offsets, HIPCOMP_TYPE_INT);
      m.place_parquet_strings(call.src_ptrs.p, call.src_bytes.p, mid_consumed.p, call.off_ptrs.p, mid_counts.p, call.level_ptrs.p, call.rows.p,
                              call.max_levels.p, reinterpret_cast<int32_t* const*>(call.out0.p), call.cap_a.p, call.out1.p, call.cap_b.p,
                              byte_counts.p, call.validity.p, status.p, n, hipcomp::ParquetStringLayout::Packed);
    }
    HIP_OK(hipStreamSynchronize(stream));
  }
  HIP_OK(hipStreamDestroy(stream));
  std::vector<uint8_t> got;
  out.download(got);
  const std::vector<hipcompStatus_t> ls = lvl_status.get(), ms = mid_status.get(), st = status.get();
  const std::vector<size_t> nn = non_null.get(), mc = mid_counts.get(), bc = byte_counts.get();
  const bool has_mid = kind == 'D' || kind == 'S';
  std::ofstream dump(out_path, std::ios::binary);
  for (size_t k = 0; k < n; ++k) {
    const Item& it = items[k];
    std::printf("page %zu levels_status %d mid_status %d status %d non_null %zu mid_count %lld count %lld guards %d\n", k, (int)ls[k],
                has_mid ? (int)ms[k] : 0, (int)st[k], nn[k], has_mid ? (long long)mc[k] : -1ll, kind == 'S' ? (long long)bc[k] : -1ll,
                (int)guards_of(it, got));
    dump.write(reinterpret_cast<const char*>(got.data() + out_levels[k]), (std::streamsize)it.rows);
    for (int o = 0; o < it.outs; ++o)
      dump.write(reinterpret_cast<const char*>(got.data() + it.out[o]), (std::streamsize)it.out_bytes[o]);
  }
  return 0;
}

template <class F>
static int throws(F f)
{
  try {
    f();
  } catch (const std::runtime_error&) {
    return 1;
  }
  return 0;
}

static int misuse()
{
  using VL = hipcomp::ParquetValueLayout;
  using SL = hipcomp::ParquetStringLayout;
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  int threw = 0, quiet = 0, worked = 0, nothing_launched = 0;
  {
    hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
    // a real item of each call: the body "ab" "" as len32 bytes len32 bytes, two values, three rows, the second null
    const uint8_t body[] = {2, 0, 0, 0, 'a', 'b', 0, 0, 0, 0, 0, 0};
    const int32_t offsets[] = {0, 2, 2};
    const uint8_t levels[] = {1, 0, 1};
    Arena a;
    const size_t at_body = a.place(sizeof(body), 0, false), at_off = a.place(sizeof(offsets), 0, false), at_lvl = a.place(3, 0, false);
    std::memcpy(a.host.data() + at_body, body, sizeof(body));
    std::memcpy(a.host.data() + at_off, offsets, sizeof(offsets));
    std::memcpy(a.host.data() + at_lvl, levels, 3);
    const size_t at_out = a.place(16, 0, false), at_bytes = a.place(8, 0, false), at_valid = a.place(1, 0, false);
    a.upload();
    const DeviceArray<const uint8_t*> src(std::vector<const uint8_t*>{a.dev + at_body}), lvl(std::vector<const uint8_t*>{a.dev + at_lvl});
    const DeviceArray<const int32_t*> off(std::vector<const int32_t*>{reinterpret_cast<const int32_t*>(a.dev + at_off)});
    const DeviceArray<int32_t*> out_off(std::vector<int32_t*>{reinterpret_cast<int32_t*>(a.dev + at_out)});
    const DeviceArray<void*> out(std::vector<void*>{a.dev + at_out});
    const DeviceArray<uint8_t*> bits(std::vector<uint8_t*>{a.dev + at_out}), bytes(std::vector<uint8_t*>{a.dev + at_bytes}),
        valid(std::vector<uint8_t*>{a.dev + at_valid});
    const DeviceArray<size_t> twelve(std::vector<size_t>{12}), two(std::vector<size_t>{2}), three(std::vector<size_t>{3}),
        four(std::vector<size_t>{4}), eight(std::vector<size_t>{8}), zero(std::vector<size_t>{0});
    const DeviceArray<uint32_t> one(std::vector<uint32_t>{1});
    DeviceArray<hipcompStatus_t> st(4, 0x77);
    const size_t many = (size_t(1) << 20) + 1;
    // place_parquet_values: too many items, value_bytes of 0 and of 65, an unknown layout, each mandatory array null, the levels'
    // arrays apart
    auto values = [&](const uint8_t* const* s, const size_t* sb, const size_t* nv, const uint8_t* const* lv, const size_t* nr, const uint32_t* ml,
                      void* const* o, const size_t* oc, hipcompStatus_t* status, size_t n, uint32_t w, VL layout) {
      m.place_parquet_values(s, sb, zero.p, nv, lv, nr, ml, o, oc, valid.p, status, n, w, layout);
    };
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, many, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 0, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 65, VL::ByteStreamSplit); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 4, (VL)2); });
    threw += throws([&] { values(nullptr, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, nullptr, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, nullptr, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, nullptr, three.p, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, nullptr, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, nullptr, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, nullptr, nullptr, out.p, three.p, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, lvl.p, three.p, nullptr, out.p, three.p, st.p, 1, 4, VL::Plain); });
    threw += throws([&] { values(src.p, twelve.p, two.p, nullptr, nullptr, one.p, out.p, three.p, st.p, 1, 4, VL::Plain); });
    // place_parquet_booleans: too many items, each mandatory array null, the levels' arrays apart
    auto booleans = [&](const uint8_t* const* s, const size_t* sb, const size_t* nv, const uint8_t* const* lv, const size_t* nr,
                        const uint32_t* ml, uint8_t* const* o, const size_t* oc, hipcompStatus_t* status, size_t n) {
      m.place_parquet_booleans(s, sb, zero.p, nv, lv, nr, ml, o, oc, valid.p, status, n);
    };
    hipcompStatus_t* const s1 = st.p + 1;
    threw += throws([&] { booleans(src.p, twelve.p, two.p, lvl.p, three.p, one.p, bits.p, three.p, s1, many); });
    threw += throws([&] { booleans(nullptr, twelve.p, two.p, lvl.p, three.p, one.p, bits.p, three.p, s1, 1); });
    threw += throws([&] { booleans(src.p, nullptr, two.p, lvl.p, three.p, one.p, bits.p, three.p, s1, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, nullptr, lvl.p, three.p, one.p, bits.p, three.p, s1, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, two.p, lvl.p, three.p, one.p, nullptr, three.p, s1, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, two.p, lvl.p, three.p, one.p, bits.p, nullptr, s1, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, two.p, lvl.p, three.p, one.p, bits.p, three.p, nullptr, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, two.p, lvl.p, nullptr, nullptr, bits.p, three.p, s1, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, two.p, lvl.p, three.p, nullptr, bits.p, three.p, s1, 1); });
    threw += throws([&] { booleans(src.p, twelve.p, two.p, nullptr, three.p, one.p, bits.p, three.p, s1, 1); });
    // place_parquet_strings: too many items, an unknown layout, each mandatory array null, the levels' arrays apart
    auto strings = [&](const uint8_t* const* s, const size_t* sb, const int32_t* const* of, const size_t* nv, const uint8_t* const* lv,
                       const size_t* nr, const uint32_t* ml, int32_t* const* oo, const size_t* oc, uint8_t* const* ob, const size_t* bc,
                       hipcompStatus_t* status, size_t n, SL layout) {
      m.place_parquet_strings(s, sb, zero.p, of, nv, lv, nr, ml, oo, oc, ob, bc, nullptr, valid.p, status, n, layout);
    };
    hipcompStatus_t* const s2 = st.p + 2;
    const SL lp = SL::LengthPrefixed;
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, many, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1, (SL)2); });
    threw += throws([&] { strings(nullptr, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, nullptr, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, nullptr, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, nullptr, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, nullptr, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, nullptr, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, nullptr, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, nullptr, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, nullptr, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, nullptr, nullptr, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, nullptr, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    threw += throws([&] { strings(src.p, twelve.p, off.p, two.p, nullptr, three.p, nullptr, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp); });
    HIP_OK(hipStreamSynchronize(stream));
    std::vector<uint8_t> after;
    a.download(after);
    nothing_launched = after == a.host;
    for (const hipcompStatus_t s : st.get())
      nothing_launched = nothing_launched && (uint32_t)s == 0x77777777u;
    // no items: nothing to do, whatever the arrays
    quiet += 1 - throws([&] {
      m.place_parquet_values(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 4, VL::Plain);
    });
    quiet += 1 - throws([&] {
      m.place_parquet_booleans(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    });
    quiet += 1 - throws([&] {
      m.place_parquet_strings(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, 0, SL::Packed);
    });
    // and the calls as they are meant: "ab" null "" as strings; the body's first two words as three values of 4 bytes; its first three
    // bits (0 1 0: the byte is 2) as "false null true"
    strings(src.p, twelve.p, off.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1, lp);
    HIP_OK(hipStreamSynchronize(stream));
    a.download(after);
    const int32_t want_rows[] = {0, 2, 2, 2};
    worked += std::memcmp(after.data() + at_out, want_rows, 16) == 0 && std::memcmp(after.data() + at_bytes, "ab", 2) == 0 && after[at_valid] == 5;
    values(src.p, twelve.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p, 1, 4, VL::Plain);
    HIP_OK(hipStreamSynchronize(stream));
    a.download(after);
    const uint8_t want_values[] = {2, 0, 0, 0, 0, 0, 0, 0, 'a', 'b', 0, 0};
    worked += std::memcmp(after.data() + at_out, want_values, 12) == 0 && after[at_valid] == 5;
    booleans(src.p, twelve.p, two.p, lvl.p, three.p, one.p, bits.p, three.p, s1, 1);
    HIP_OK(hipStreamSynchronize(stream));
    a.download(after);
    worked += after[at_out] == 4 && after[at_out + 1] == 0 && after[at_valid] == 5;
    const std::vector<hipcompStatus_t> s = st.get();
    worked += s[0] == hipcompSuccess && s[1] == hipcompSuccess && s[2] == hipcompSuccess;
  }
  HIP_OK(hipStreamDestroy(stream));
  std::printf("threw %d nothing_launched %d quiet %d worked %d\n", threw, nothing_launched, quiet, worked);
  return 0;
}

#ifdef PLAIN_HOST_PATH
//   parquet_plain_driver time POOL LIST reps     (scripts/quick_parquet_plain.py; built with -DPLAIN_HOST_PATH)
// LIST: one case.  Three ways, alternating inside every repetition, HIP events around each, 2 warm-ups, medians: the one
// call; one device-to-device copy of as many bytes as the outputs take; and today's way -- every input copied to the host
// in one copy, the items worked there by one thread with the functions of parquet_plain_plan.hpp, the outputs copied back
// in one copy.  same: the call and the host wrote the same bytes and every status is success.
static float median(std::vector<float> v)
{
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

static int time_case(const char* pool_path, const char* list_path, int reps)
{
  using namespace hcamd::pqv;
  const std::vector<uint8_t> pool = read_file(pool_path);
  std::ifstream list(list_path);
  std::string line, word, kind, out_path;
  uint32_t value_bytes, layout;
  int has_levels, nulls, ones;
  size_t align, n;
  std::getline(list, line);
  std::istringstream ls(line);
  if (!(ls >> word >> kind >> value_bytes >> layout >> has_levels >> align >> nulls >> ones >> out_path >> n) || word != "case")
    return 2;
  std::vector<Item> items(n);
  Arena in, out;
  size_t out_bytes = 0, rows = 0;
  for (size_t k = 0; k < n; ++k) {
    if (!std::getline(list, line) || !parse_item(line, items[k]))
      return 2;
    lay_out(items[k], pool, in, out, align);
    rows += items[k].rows;
    for (int o = 0; o < items[k].outs; ++o)
      out_bytes += items[k].out_bytes[o];
  }
  in.upload();
  out.upload();
  uint8_t *copy_from, *copy_to, *host_back;
  HIP_OK(hipMalloc(&copy_from, out_bytes + 16));
  HIP_OK(hipMalloc(&copy_to, out_bytes + 16));
  HIP_OK(hipMalloc(&host_back, out.host.size() + 16));
  HIP_OK(hipMemset(copy_from, 1, out_bytes));
  std::vector<uint8_t> host_in(in.host.size()), host_out(out.host);
  DeviceArray<hipcompStatus_t> statuses(n, 0x77);
  DeviceArray<size_t> counts(n, 0x77);
  const DeviceCall call((Call(items, in, out)));
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  std::vector<float> t_call, t_copy, t_host;
  bool host_ok = true;
  {
    hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
    for (int rep = -2; rep < reps; ++rep) {
      float ms;
      HIP_OK(hipEventRecord(e0, stream));
      call.run(m, kind[0], value_bytes, layout, has_levels != 0, nulls, 0, n, statuses.p, counts.p);
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 0)
        t_call.push_back(ms);
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(hipMemcpyAsync(copy_to, copy_from, out_bytes, hipMemcpyDeviceToDevice, stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 0)
        t_copy.push_back(ms);
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(hipMemcpyAsync(host_in.data(), in.dev, host_in.size(), hipMemcpyDeviceToHost, stream));
      HIP_OK(hipStreamSynchronize(stream));
      for (const Item& it : items) {
        const uint8_t* const src = host_in.data() + it.in_src;
        const Rows r = rows_of(it.num_values, it.has_levels ? host_in.data() + it.in_lvl : nullptr, it.rows, (uint32_t)it.max_level);
        if (it.kind == 'V')
          host_ok = place_values_item(src, it.src_bytes, it.start, r, it.cap_a, (uint32_t)it.value_bytes, (uint32_t)it.layout,
                                      host_out.data() + it.out[0], host_out.data() + it.out[1])
                    && host_ok;
        else if (it.kind == 'B')
          host_ok = place_booleans_item(src, it.src_bytes, it.start, r, it.cap_a, host_out.data() + it.out[0], host_out.data() + it.out[1])
                    && host_ok;
        else
          host_ok = place_strings_item(src, it.src_bytes, it.start, reinterpret_cast<const int32_t*>(host_in.data() + it.in_off), r,
                                       (uint32_t)it.layout, it.cap_a, it.cap_b, reinterpret_cast<int32_t*>(host_out.data() + it.out[0]),
                                       host_out.data() + it.out[1], host_out.data() + it.out[2])
                        .ok
                    && host_ok;
      }
      HIP_OK(hipMemcpyAsync(host_back, host_out.data(), host_out.size(), hipMemcpyHostToDevice, stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 0)
        t_host.push_back(ms);
    }
  }
  std::vector<uint8_t> got;
  out.download(got);
  bool same = host_ok && got == host_out;
  for (const hipcompStatus_t s : statuses.get())
    same = same && s == hipcompSuccess;
  std::printf("items %zu rows %zu in_bytes %zu out_bytes %zu same %d call_ms %.4f copy_ms %.4f host_ms %.4f reps %d\n", n, rows,
              in.host.size(), out_bytes, (int)same, median(t_call), median(t_copy), median(t_host), reps);
  (void)hipFree(copy_from);
  (void)hipFree(copy_to);
  (void)hipFree(host_back);
  HIP_OK(hipStreamDestroy(stream));
  return 0;
}
#endif

int main(int argc, char** argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "batch" && argc == 4)
    return batch(argv[2], argv[3]);
  if (mode == "chain" && argc == 9)
    return chain(argv[2], argv[3], argv[4], std::atoi(argv[5]), argv[6][0], (uint32_t)std::atoi(argv[7]), (uint32_t)std::atoi(argv[8]));
  if (mode == "misuse" && argc == 2)
    return misuse();
#ifdef PLAIN_HOST_PATH
  if (mode == "time" && argc == 5)
    return time_case(argv[2], argv[3], std::atoi(argv[4]));
#endif
  std::fprintf(stderr, "usage: %s batch POOL LIST | chain POOL LIST OUT form KIND value_bytes layout | misuse\n", argv[0]);
  return 2;
}
