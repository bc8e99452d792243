// parquet_dict_driver.cpp -- the three calls that gather a Parquet dictionary's entries to rows (hipcomp/cascaded.hpp:
// index_parquet_dictionary, gather_parquet_dictionary, gather_parquet_dictionary_strings), driven for
// tests/test_parquet_dict_gpu.py: a C++ program written against include/ and linked to libhipcomp.so.
//
//   parquet_dict_driver batch POOL LIST
// LIST: "case KIND entry_bytes has_levels align nulls ones OUT items", then a line per item as
// tests/parquet_dictgen.py's Item.line writes it (places and lengths in POOL).  A case is one call.  Every output has 32
// guard bytes on both sides; with `align`, dictionaries, validity arrays and string bytes lie that many bytes behind an
// aligned address and the other outputs at the alignment the contract states, no better.  nulls: 1
// without the count array, 2 without the validity array.  ones: every item is also worked in a call of its own, into
// outputs of its own, and compared.  Per item "item k status s count c guards g (c: -1 where the call has no count array) [one_status s one_count c eq_one e]",
// then "case n"; OUT gets every output of every item, the whole capacity, back to back.
//
//   parquet_dict_driver chain POOL LIST OUT form entry_bytes
// LIST: a line per page, "levels length indices length rows dict length entries": the levels, then the indices with the
// levels' match counts as their num_values, then (entry_bytes 0: strings) the dictionary's offsets, then the gather with
// those match counts as its device_num_indices and the index call's entry counts as its device_dict_entries; nothing is
// read back and nothing waits between the calls.  OUT: per page the levels, then the outputs as above.
//
//   parquet_dict_driver misuse
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
#ifdef DICT_HOST_PATH
#include <algorithm>

#include "parquet_dict_plan.hpp" // the host path of `time`: what a user without the calls runs
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
  std::map<std::pair<uint64_t, uint64_t>, size_t> shared; // the dictionaries put so far: (place in the pool, bytes) -> place here
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
  char kind = 'I';
  uint64_t dict_at = 0, dict_bytes = 0, entries = 0, doff_at = 0, doff_count = 0, idx_at = 0, num_indices = 0, has_levels = 0, lvl_at = 0,
           rows = 0, max_level = 0, cap_a = 0, cap_b = 0;
  size_t in_dict = 0, in_doff = 0, in_idx = 0, in_lvl = 0;
  size_t out[3] = {0, 0, 0}, out_bytes[3] = {0, 0, 0};
  int outs = 0;
};

static bool parse_item(const std::string& line, Item& it)
{
  std::istringstream ls(line);
  std::string kind;
  if (!(ls >> kind >> it.dict_at >> it.dict_bytes >> it.entries) || kind.size() != 1)
    return false;
  it.kind = kind[0];
  if (it.kind == 'I')
    return (bool)(ls >> it.cap_a);
  if (it.kind == 'S' && !(ls >> it.doff_at >> it.doff_count))
    return false;
  return (bool)(ls >> it.idx_at >> it.num_indices >> it.has_levels >> it.lvl_at >> it.rows >> it.max_level >> it.cap_a >> it.cap_b);
}

// With `align`, an output lies at the alignment the contract states and no better: an odd multiple of it.
static size_t stated(size_t align, size_t element_bytes)
{
  size_t a = 1;
  while (a < 8 && element_bytes % (2 * a) == 0)
    a *= 2;
  return align ? a : 0;
}

static void lay_out(Item& it, const std::vector<uint8_t>& pool, Arena& in, Arena& out, size_t align)
{
  // (items that name the same bytes of the pool share one dictionary, as the pages of a column chunk do)
  const auto key = std::make_pair(it.dict_at, it.dict_bytes);
  if (!in.shared.count(key))
    in.shared[key] = in.put(pool, it.dict_at, it.dict_bytes, align);
  it.in_dict = in.shared[key];
  const size_t validity = (it.rows + 7) / 8;
  if (it.kind == 'I') {
    it.outs = 1;
    it.out_bytes[0] = 4 * it.cap_a;
    it.out[0] = out.place(it.out_bytes[0], stated(align, 4), true);
    return;
  }
  it.in_idx = in.put(pool, it.idx_at, 4 * it.num_indices, 0);
  it.in_lvl = in.put(pool, it.lvl_at, it.has_levels ? it.rows : 0, 0);
  if (it.kind == 'F') {
    it.outs = 2;
    it.out_bytes[0] = it.cap_a * it.cap_b;
    it.out[0] = out.place(it.out_bytes[0], stated(align, it.cap_b), true);
    it.out_bytes[1] = validity;
    it.out[1] = out.place(validity, align, true);
  } else {
    it.in_doff = in.put(pool, it.doff_at, 4 * it.doff_count, 0);
    it.outs = 3;
    it.out_bytes[0] = 4 * it.cap_a;
    it.out[0] = out.place(it.out_bytes[0], stated(align, 4), true);
    it.out_bytes[1] = it.cap_b;
    it.out[1] = out.place(it.out_bytes[1], align, true);
    it.out_bytes[2] = validity;
    it.out[2] = out.place(validity, align, true);
  }
}

// the device arrays of a call over items [0, n), outputs in `out`
struct Call
{
  std::vector<const uint8_t*> dict_ptrs, level_ptrs;
  std::vector<size_t> dict_bytes, entries, num_indices, rows, cap_a, cap_b;
  std::vector<const uint32_t*> index_ptrs;
  std::vector<const int32_t*> doff_ptrs;
  std::vector<uint32_t> max_levels;
  std::vector<void*> out0;
  std::vector<uint8_t*> out1, validity;
  Call(const std::vector<Item>& items, const Arena& in, const Arena& out)
  {
    for (const Item& it : items) {
      dict_ptrs.push_back(in.dev + it.in_dict);
      dict_bytes.push_back(it.dict_bytes);
      entries.push_back(it.entries);
      index_ptrs.push_back(reinterpret_cast<const uint32_t*>(in.dev + it.in_idx));
      num_indices.push_back(it.num_indices);
      level_ptrs.push_back(in.dev + it.in_lvl);
      rows.push_back(it.rows);
      max_levels.push_back((uint32_t)it.max_level);
      doff_ptrs.push_back(reinterpret_cast<const int32_t*>(in.dev + it.in_doff));
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
  DeviceArray<const uint8_t*> dict_ptrs, level_ptrs;
  DeviceArray<size_t> dict_bytes, entries, num_indices, rows, cap_a, cap_b;
  DeviceArray<const uint32_t*> index_ptrs;
  DeviceArray<const int32_t*> doff_ptrs;
  DeviceArray<uint32_t> max_levels;
  DeviceArray<void*> out0;
  DeviceArray<uint8_t*> out1, validity;
  explicit DeviceCall(const Call& c)
      : dict_ptrs(c.dict_ptrs), level_ptrs(c.level_ptrs), dict_bytes(c.dict_bytes), entries(c.entries), num_indices(c.num_indices),
        rows(c.rows), cap_a(c.cap_a), cap_b(c.cap_b), index_ptrs(c.index_ptrs), doff_ptrs(c.doff_ptrs), max_levels(c.max_levels),
        out0(c.out0), out1(c.out1), validity(c.validity)
  {
  }
  // items [first, first + n) in one call
  void run(hipcomp::CascadedManager& m, char kind, uint32_t entry_bytes, bool has_levels, int nulls, size_t first, size_t n,
           hipcompStatus_t* statuses, size_t* counts) const
  {
    size_t* const count = (nulls & 1) ? nullptr : counts + first;
    uint8_t* const* const valid = (nulls & 2) ? nullptr : validity.p + first;
    const uint8_t* const* const levels = has_levels ? level_ptrs.p + first : nullptr;
    const size_t* const num_rows = has_levels ? rows.p + first : nullptr;
    const uint32_t* const maxima = has_levels ? max_levels.p + first : nullptr;
    if (kind == 'I')
      m.index_parquet_dictionary(dict_ptrs.p + first, dict_bytes.p + first, entries.p + first, reinterpret_cast<int32_t* const*>(out0.p + first),
                                 cap_a.p + first, count, statuses + first, n);
    else if (kind == 'F')
      m.gather_parquet_dictionary(dict_ptrs.p + first, dict_bytes.p + first, entries.p + first, index_ptrs.p + first, num_indices.p + first,
                                  levels, num_rows, maxima, out0.p + first, cap_a.p + first, valid, statuses + first, n, entry_bytes);
    else
      m.gather_parquet_dictionary_strings(dict_ptrs.p + first, dict_bytes.p + first, entries.p + first, doff_ptrs.p + first,
                                          index_ptrs.p + first, num_indices.p + first, levels, num_rows, maxima,
                                          reinterpret_cast<int32_t* const*>(out0.p + first), cap_a.p + first, out1.p + first, cap_b.p + first,
                                          count, valid, statuses + first, n);
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
      uint32_t entry_bytes;
      int has_levels, nulls, ones;
      size_t align, n;
      if (!(ls >> word >> kind >> entry_bytes >> has_levels >> align >> nulls >> ones >> out_path >> n) || word != "case") {
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
        lay_out(items[k], pool, in, out, align);
      }
      alone.host = out.host;
      in.upload();
      out.upload();
      const uint8_t status_fill = 0x77;
      DeviceArray<hipcompStatus_t> statuses(n, status_fill), one_statuses(n, status_fill);
      DeviceArray<size_t> counts(n, status_fill), one_counts(n, status_fill);
      const DeviceCall call((Call(items, in, out)));
      call.run(manager, kind[0], entry_bytes, has_levels != 0, nulls, 0, n, statuses.p, counts.p);
      HIP_OK(hipStreamSynchronize(stream));
      std::vector<uint8_t> got, got_alone;
      out.download(got);
      if (ones) {
        alone.upload();
        const DeviceCall each((Call(items, in, alone)));
        for (size_t k = 0; k < n; ++k)
          each.run(manager, kind[0], entry_bytes, has_levels != 0, nulls, k, 1, one_statuses.p, one_counts.p);
        HIP_OK(hipStreamSynchronize(stream));
        alone.download(got_alone);
      }
      const std::vector<hipcompStatus_t> st = statuses.get(), one_st = one_statuses.get();
      const std::vector<size_t> ct = counts.get(), one_ct = one_counts.get();
      std::ofstream dump(out_path, std::ios::binary);
      const bool no_count = (nulls & 1) || kind[0] == 'F'; // (the fixed-width gather reports no count)
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

static int chain(const char* pool_path, const char* list_path, const char* out_path, int form, uint32_t entry_bytes)
{
  const std::vector<uint8_t> pool = read_file(pool_path);
  std::ifstream list(list_path);
  std::string line;
  std::vector<Item> items;
  std::vector<size_t> lvl_bytes, idx_bytes;
  Arena in, out;
  std::vector<size_t> in_lvl_stream, in_idx_stream, out_levels, out_indices;
  while (std::getline(list, line)) {
    std::istringstream ls(line);
    uint64_t la, ll, ia, il;
    Item it;
    if (!(ls >> la >> ll >> ia >> il >> it.rows >> it.dict_at >> it.dict_bytes >> it.entries)) {
      std::fprintf(stderr, "bad page: %s\n", line.c_str());
      return 2;
    }
    it.kind = entry_bytes ? 'F' : 'S';
    it.has_levels = 1;
    it.max_level = 1;
    it.cap_a = entry_bytes ? it.rows : it.rows + 1;
    it.cap_b = entry_bytes ? entry_bytes : 400 * it.rows; // (no fixture string is longer)
    in_lvl_stream.push_back(in.put(pool, la, ll, 0));
    in_idx_stream.push_back(in.put(pool, ia, il, 0));
    lvl_bytes.push_back(ll);
    idx_bytes.push_back(il);
    lay_out(it, pool, in, out, 1);
    // what the hybrid calls write, and the index call: outputs too, but of this program's own
    out_levels.push_back(out.place(it.rows, 0, true));
    out_indices.push_back(out.place(4 * it.rows, 0, true));
    it.in_doff = out.place(4 * (it.entries + 1), 0, true); // (in `out`: the index call writes it)
    items.push_back(it);
  }
  const size_t n = items.size();
  in.upload();
  out.upload();
  Call c(items, in, out);
  std::vector<const uint8_t*> lvl_streams, idx_streams;
  std::vector<void*> lvl_outs, idx_outs;
  std::vector<int32_t*> doff_outs;
  std::vector<size_t> doff_caps;
  for (size_t k = 0; k < n; ++k) {
    lvl_streams.push_back(in.dev + in_lvl_stream[k]);
    idx_streams.push_back(in.dev + in_idx_stream[k]);
    lvl_outs.push_back(out.dev + out_levels[k]);
    idx_outs.push_back(out.dev + out_indices[k]);
    c.level_ptrs[k] = out.dev + out_levels[k];
    c.index_ptrs[k] = reinterpret_cast<const uint32_t*>(out.dev + out_indices[k]);
    c.doff_ptrs[k] = reinterpret_cast<const int32_t*>(out.dev + items[k].in_doff);
    doff_outs.push_back(reinterpret_cast<int32_t*>(out.dev + items[k].in_doff));
    doff_caps.push_back(items[k].entries + 1);
  }
  const DeviceCall call(c);
  const DeviceArray<const uint8_t*> d_lvl_streams(lvl_streams), d_idx_streams(idx_streams);
  const DeviceArray<void*> d_lvl_outs(lvl_outs), d_idx_outs(idx_outs);
  const DeviceArray<int32_t*> d_doff_outs(doff_outs);
  const DeviceArray<size_t> d_lvl_bytes(lvl_bytes), d_idx_bytes(idx_bytes), d_doff_caps(doff_caps);
  const DeviceArray<uint32_t> ones(std::vector<uint32_t>(n, 1u));
  const uint8_t fill = 0x77;
  DeviceArray<size_t> non_null(n, fill), entry_counts(n, fill), byte_counts(n, fill);
  DeviceArray<hipcompStatus_t> lvl_status(n, fill), idx_status(n, fill), dict_status(n, fill), status(n, fill);
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  {
    hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
    // nothing is read back and nothing waits between these calls
    m.decode_parquet_hybrid(d_lvl_streams.p, d_lvl_bytes.p, ones.p, call.rows.p, d_lvl_outs.p, call.rows.p, nullptr, ones.p, non_null.p,
                            lvl_status.p, n, (hipcomp::ParquetHybridForm)form, HIPCOMP_TYPE_UCHAR);
    m.decode_parquet_hybrid(d_idx_streams.p, d_idx_bytes.p, nullptr, non_null.p, d_idx_outs.p, call.rows.p, nullptr, nullptr, nullptr,
                            idx_status.p, n, hipcomp::ParquetHybridForm::WidthPrefixed, HIPCOMP_TYPE_UINT);
    if (entry_bytes) {
      m.gather_parquet_dictionary(call.dict_ptrs.p, call.dict_bytes.p, call.entries.p, call.index_ptrs.p, non_null.p, call.level_ptrs.p,
                                  call.rows.p, call.max_levels.p, call.out0.p, call.cap_a.p, call.validity.p, status.p, n, entry_bytes);
    } else {
      m.index_parquet_dictionary(call.dict_ptrs.p, call.dict_bytes.p, call.entries.p, d_doff_outs.p, d_doff_caps.p, entry_counts.p,
                                 dict_status.p, n);
      m.gather_parquet_dictionary_strings(call.dict_ptrs.p, call.dict_bytes.p, entry_counts.p, call.doff_ptrs.p, call.index_ptrs.p,
                                          non_null.p, call.level_ptrs.p, call.rows.p, call.max_levels.p,
                                          reinterpret_cast<int32_t* const*>(call.out0.p), call.cap_a.p, call.out1.p, call.cap_b.p,
                                          byte_counts.p, call.validity.p, status.p, n);
    }
    HIP_OK(hipStreamSynchronize(stream));
  }
  HIP_OK(hipStreamDestroy(stream));
  std::vector<uint8_t> got;
  out.download(got);
  const std::vector<hipcompStatus_t> ls = lvl_status.get(), is = idx_status.get(), ds = dict_status.get(), st = status.get();
  const std::vector<size_t> nn = non_null.get(), ec = entry_counts.get(), bc = byte_counts.get();
  std::ofstream dump(out_path, std::ios::binary);
  for (size_t k = 0; k < n; ++k) {
    const Item& it = items[k];
    std::printf("page %zu levels_status %d indices_status %d dictionary_status %d status %d non_null %zu entries %lld count %lld guards %d\n",
                k, (int)ls[k], (int)is[k], entry_bytes ? 0 : (int)ds[k], (int)st[k], nn[k], entry_bytes ? -1ll : (long long)ec[k],
                entry_bytes ? -1ll : (long long)bc[k], (int)guards_of(it, got));
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
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  int threw = 0, quiet = 0, worked = 0, nothing_launched = 0;
  {
    hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
    // a real item of each call: a dictionary of two entries, "ab" and "", three rows, the second null
    const uint8_t body[] = {2, 0, 0, 0, 'a', 'b', 0, 0, 0, 0, 0, 0};
    const uint32_t indices[] = {1, 0};
    const uint8_t levels[] = {1, 0, 1};
    Arena a;
    const size_t at_body = a.place(sizeof(body), 0, false), at_idx = a.place(sizeof(indices), 0, false), at_lvl = a.place(3, 0, false);
    std::memcpy(a.host.data() + at_body, body, sizeof(body));
    std::memcpy(a.host.data() + at_idx, indices, sizeof(indices));
    std::memcpy(a.host.data() + at_lvl, levels, 3);
    const size_t at_off = a.place(12, 0, false), at_out = a.place(16, 0, false), at_bytes = a.place(8, 0, false), at_valid = a.place(1, 0, false);
    a.upload();
    const DeviceArray<const uint8_t*> dict(std::vector<const uint8_t*>{a.dev + at_body}), lvl(std::vector<const uint8_t*>{a.dev + at_lvl});
    const DeviceArray<const uint32_t*> idx(std::vector<const uint32_t*>{reinterpret_cast<const uint32_t*>(a.dev + at_idx)});
    const DeviceArray<int32_t*> off(std::vector<int32_t*>{reinterpret_cast<int32_t*>(a.dev + at_off)});
    const DeviceArray<const int32_t*> coff(std::vector<const int32_t*>{reinterpret_cast<const int32_t*>(a.dev + at_off)});
    const DeviceArray<int32_t*> out_off(std::vector<int32_t*>{reinterpret_cast<int32_t*>(a.dev + at_out)});
    const DeviceArray<void*> out(std::vector<void*>{a.dev + at_out});
    const DeviceArray<uint8_t*> bytes(std::vector<uint8_t*>{a.dev + at_bytes}), valid(std::vector<uint8_t*>{a.dev + at_valid});
    const DeviceArray<size_t> twelve(std::vector<size_t>{12}), two(std::vector<size_t>{2}), three(std::vector<size_t>{3}),
        four(std::vector<size_t>{4}), eight(std::vector<size_t>{8});
    const DeviceArray<uint32_t> one(std::vector<uint32_t>{1});
    DeviceArray<hipcompStatus_t> st(4, 0x77);
    const size_t many = (size_t(1) << 20) + 1;
    // index_parquet_dictionary: too many items, each mandatory array null
    threw += throws([&] { m.index_parquet_dictionary(dict.p, twelve.p, two.p, off.p, three.p, nullptr, st.p, many); });
    threw += throws([&] { m.index_parquet_dictionary(nullptr, twelve.p, two.p, off.p, three.p, nullptr, st.p, 1); });
    threw += throws([&] { m.index_parquet_dictionary(dict.p, nullptr, two.p, off.p, three.p, nullptr, st.p, 1); });
    threw += throws([&] { m.index_parquet_dictionary(dict.p, twelve.p, nullptr, off.p, three.p, nullptr, st.p, 1); });
    threw += throws([&] { m.index_parquet_dictionary(dict.p, twelve.p, two.p, nullptr, three.p, nullptr, st.p, 1); });
    threw += throws([&] { m.index_parquet_dictionary(dict.p, twelve.p, two.p, off.p, nullptr, nullptr, st.p, 1); });
    threw += throws([&] { m.index_parquet_dictionary(dict.p, twelve.p, two.p, off.p, three.p, nullptr, nullptr, 1); });
    // gather_parquet_dictionary: too many items, entry_bytes of 0 and of 65, each mandatory array null, the levels' arrays apart
    auto fixed = [&](const uint8_t* const* d, const size_t* db, const size_t* de, const uint32_t* const* ix, const size_t* ni,
                     const uint8_t* const* lv, const size_t* nr, const uint32_t* ml, void* const* o, const size_t* oc, hipcompStatus_t* s,
                     size_t n, uint32_t e) { m.gather_parquet_dictionary(d, db, de, ix, ni, lv, nr, ml, o, oc, valid.p, s, n, e); };
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, many, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 0); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 65); });
    threw += throws([&] { fixed(nullptr, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, nullptr, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, nullptr, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, nullptr, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, nullptr, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, nullptr, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, nullptr, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, nullptr, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, nullptr, nullptr, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, nullptr, out.p, three.p, st.p + 1, 1, 4); });
    threw += throws([&] { fixed(dict.p, twelve.p, three.p, idx.p, two.p, nullptr, nullptr, one.p, out.p, three.p, st.p + 1, 1, 4); });
    // gather_parquet_dictionary_strings: too many items, each mandatory array null, the levels alone
    auto strings = [&](const uint8_t* const* d, const size_t* db, const size_t* de, const int32_t* const* dof, const uint32_t* const* ix,
                       const size_t* ni, const uint8_t* const* lv, const size_t* nr, const uint32_t* ml, int32_t* const* oo, const size_t* oc,
                       uint8_t* const* ob, const size_t* bc, hipcompStatus_t* s, size_t n) {
      m.gather_parquet_dictionary_strings(d, db, de, dof, ix, ni, lv, nr, ml, oo, oc, ob, bc, nullptr, valid.p, s, n);
    };
    hipcompStatus_t* const s2 = st.p + 2;
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, many); });
    threw += throws([&] { strings(nullptr, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, nullptr, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, nullptr, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, nullptr, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, nullptr, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, nullptr, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, nullptr, four.p, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, nullptr, bytes.p, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, nullptr, eight.p, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, nullptr, s2, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, nullptr, 1); });
    threw += throws([&] { strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, nullptr, nullptr, out_off.p, four.p, bytes.p, eight.p, s2, 1); });
    HIP_OK(hipStreamSynchronize(stream));
    std::vector<uint8_t> after;
    a.download(after);
    nothing_launched = after == a.host;
    for (const hipcompStatus_t s : st.get())
      nothing_launched = nothing_launched && (uint32_t)s == 0x77777777u;
    // no items: nothing to do, whatever the arrays
    quiet += 1 - throws([&] { m.index_parquet_dictionary(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0); });
    quiet += 1 - throws([&] {
      m.gather_parquet_dictionary(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 4);
    });
    quiet += 1 - throws([&] {
      m.gather_parquet_dictionary_strings(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    });
    // and the calls as they are meant: the offsets, then "" null "ab" as strings, then entries 1 and 0 of the body as three of 4 bytes
    m.index_parquet_dictionary(dict.p, twelve.p, two.p, off.p, three.p, nullptr, st.p, 1);
    strings(dict.p, twelve.p, two.p, coff.p, idx.p, two.p, lvl.p, three.p, one.p, out_off.p, four.p, bytes.p, eight.p, s2, 1);
    HIP_OK(hipStreamSynchronize(stream));
    a.download(after);
    const int32_t want_off[] = {0, 2, 2}, want_rows[] = {0, 0, 0, 2};
    worked += std::memcmp(after.data() + at_off, want_off, 12) == 0 && std::memcmp(after.data() + at_out, want_rows, 16) == 0
              && std::memcmp(after.data() + at_bytes, "ab", 2) == 0 && after[at_valid] == 5;
    fixed(dict.p, twelve.p, three.p, idx.p, two.p, lvl.p, three.p, one.p, out.p, three.p, st.p + 1, 1, 4);
    HIP_OK(hipStreamSynchronize(stream));
    a.download(after);
    const uint8_t want_fixed[] = {'a', 'b', 0, 0, 0, 0, 0, 0, 2, 0, 0, 0};
    worked += std::memcmp(after.data() + at_out, want_fixed, 12) == 0 && after[at_valid] == 5;
    const std::vector<hipcompStatus_t> s = st.get();
    worked += s[0] == hipcompSuccess && s[1] == hipcompSuccess && s[2] == hipcompSuccess;
  }
  HIP_OK(hipStreamDestroy(stream));
  std::printf("threw %d nothing_launched %d quiet %d worked %d\n", threw, nothing_launched, quiet, worked);
  return 0;
}

#ifdef DICT_HOST_PATH
//   parquet_dict_driver time POOL LIST reps     (scripts/quick_parquet_dict.py; built with -DDICT_HOST_PATH)
// LIST: one case.  Three ways, alternating inside every repetition, HIP events around each, 2 warm-ups, medians: the one
// call; one device-to-device copy of as many bytes as the outputs take; and today's way -- every input copied to the host
// in one copy, the items worked there by one thread with the functions of parquet_dict_plan.hpp, the outputs copied back
// in one copy.  same: the call and the host wrote the same bytes and every status is success.
static float median(std::vector<float> v)
{
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

static int time_case(const char* pool_path, const char* list_path, int reps)
{
  using namespace hcamd::pqg;
  const std::vector<uint8_t> pool = read_file(pool_path);
  std::ifstream list(list_path);
  std::string line, word, kind, out_path;
  uint32_t entry_bytes;
  int has_levels, nulls, ones;
  size_t align, n;
  std::getline(list, line);
  std::istringstream ls(line);
  if (!(ls >> word >> kind >> entry_bytes >> has_levels >> align >> nulls >> ones >> out_path >> n) || word != "case")
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
      call.run(m, kind[0], entry_bytes, has_levels != 0, nulls, 0, n, statuses.p, counts.p);
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
        const uint8_t* const dict = host_in.data() + it.in_dict;
        const Rows r{reinterpret_cast<const uint32_t*>(host_in.data() + it.in_idx), it.num_indices,
                     it.has_levels ? host_in.data() + it.in_lvl : nullptr, it.rows, (uint32_t)it.max_level};
        if (it.kind == 'F')
          host_ok = gather_item(dict, it.dict_bytes, it.entries, r, it.cap_a, (uint32_t)it.cap_b, host_out.data() + it.out[0],
                                host_out.data() + it.out[1])
                    && host_ok;
        else
          host_ok = gather_strings_item(dict, it.dict_bytes, it.entries, reinterpret_cast<const int32_t*>(host_in.data() + it.in_doff), r,
                                        it.cap_a, it.cap_b, reinterpret_cast<int32_t*>(host_out.data() + it.out[0]),
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
  if (mode == "chain" && argc == 7)
    return chain(argv[2], argv[3], argv[4], std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
  if (mode == "misuse" && argc == 2)
    return misuse();
#ifdef DICT_HOST_PATH
  if (mode == "time" && argc == 5)
    return time_case(argv[2], argv[3], std::atoi(argv[4]));
#endif
  std::fprintf(stderr, "usage: %s batch POOL LIST | chain POOL LIST OUT form entry_bytes | misuse\n", argv[0]);
  return 2;
}
