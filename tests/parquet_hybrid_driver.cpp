// Batches of Parquet RLE / bit-packed hybrid streams in one call (hipcomp/cascaded.hpp: decode_parquet_hybrid of the
// Cascaded manager) driven on a GPU for tests/test_parquet_hybrid_gpu.py and scripts/quick_parquet_hybrid.py.  Written
// against include/ and linked to libhipcomp.so.
//
//   batch LIST     LIST holds cases: a line "case FORM ELEMENT ALIGN NULLS ONES OUTFILE N" and N lines
//                  "FILE OFFSET LENGTH BIT_WIDTH WANTED CAPACITY MATCH".  FORM 0 | 1 | 2 (ParquetHybridForm); ELEMENT 1 | 2 | 4
//                  bytes; ALIGN: every stream lies ALIGN bytes behind a 256-byte aligned address; NULLS: 1
//                  device_consumed_bytes is null, 2 the match arrays are, 3 both (and, under FORM 2, device_bit_widths too);
//                  ONES 1: every item is also decoded as a batch of its own, into a twin of its output.
//                  Per item a line "item I status .. consumed .. matches .. size .. guards G untouched U one_status ..
//                  one_consumed .. one_matches .. eq_one E".  size: the elements written (WANTED on success, else 0).
//                  guards: the 64 bytes on both sides of the output's CAPACITY elements, and the elements behind the `size`
//                  written ones, are as they were.  untouched: so is the whole output.  OUTFILE takes, item by item, the
//                  `size` elements.
//   chain LIST OUT the chained use: lines "FILE LEVELS_OFFSET LEVELS_LENGTH FORM INDEX_OFFSET INDEX_LENGTH ELEMENT ROWS", a
//                  page each.  One call decodes the definition levels (width 1) of all pages and counts the ones; a second
//                  call takes that device array as its num_values and decodes the indices; nothing is copied to the host or
//                  synchronised between the two.  Per page "page I levels_status .. index_status .. non_null ..
//                  index_consumed ..", OUT takes per page the ROWS levels and the non_null indices.
//   misuse         what throws before a launch
//   time LIST REPS one case line and its items: REPS alternating timings (HIP events) of the one call, of a device-to-device
//                  copy of as many bytes as it writes, and of today's way: the streams copied to the host, decoded there by
//                  one thread (the plan header's decoder), the values copied back
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "hipcomp/cascaded.hpp"
#ifdef HYBRID_HOST_DECODER
#include "parquet_hybrid_plan.hpp"
#endif

using hipcomp::ParquetHybridForm;

#define HIP(x)                                                                                          \
  do {                                                                                                  \
    const hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) {                                                                             \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);                  \
      std::exit(5);                                                                                     \
    }                                                                                                   \
  } while (0)

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kFill = 0xA5;

std::vector<uint8_t> slice_of(const std::string& file, uint64_t offset, uint64_t length)
{
  std::ifstream f(file, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", file.c_str());
    std::exit(3);
  }
  f.seekg((std::streamoff)offset);
  std::vector<uint8_t> v(length);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)length);
  if ((uint64_t)f.gcount() != length)
    std::exit(3);
  return v;
}

template <typename T>
T* device_array(size_t n)
{
  T* p = nullptr;
  HIP(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)));
  return p;
}
template <typename T>
T* device_copy(const std::vector<T>& v)
{
  T* p = device_array<T>(v.size());
  if (!v.empty())
    HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}
template <typename T>
std::vector<T> host_copy(const T* p, size_t n)
{
  std::vector<T> v(n);
  if (n)
    HIP(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
  return v;
}

size_t round_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

hipcompType_t type_of(uint32_t element)
{
  return element == 1 ? HIPCOMP_TYPE_UCHAR : element == 2 ? HIPCOMP_TYPE_USHORT : HIPCOMP_TYPE_UINT;
}

// An arena of buffers with guards around each: buffer i is [at[i], at[i] + len[i]) of the arena, `guard` bytes of
// fill on both sides, at[i] = `align` behind a multiple of 256 (`align` < 256).
struct Arena
{
  std::vector<size_t> at, len;
  size_t bytes = 0, guard = 0;
  uint8_t* dev = nullptr;
  void plan(const std::vector<size_t>& lens, size_t guard_, size_t align)
  {
    guard = guard_;
    len = lens;
    size_t pos = 0;
    for (size_t n : lens) {
      pos = round_up(pos + guard, 256) + align;
      at.push_back(pos);
      pos += n + guard;
    }
    bytes = pos + 256;
    HIP(hipMalloc((void**)&dev, bytes));
    HIP(hipMemset(dev, kFill, bytes));
  }
  ~Arena() { (void)hipFree(dev); }
};

bool all_fill(const uint8_t* p, size_t n)
{
  for (size_t i = 0; i < n; ++i)
    if (p[i] != kFill)
      return false;
  return true;
}

struct ItemSpec
{
  std::vector<uint8_t> data;
  uint32_t bit_width = 0, match = 0;
  uint64_t wanted = 0, capacity = 0;
};

struct Result
{
  std::vector<hipcompStatus_t> statuses;
  std::vector<size_t> consumed, matches;
  std::vector<uint8_t> out; // the output arena, whole
};

// one call over items [first, first + count) of the case; the streams lie in `in`, the outputs in a fresh arena
struct Call
{
  Arena out;
  Result r;
};
void run_call(hipcomp::CascadedManager& m, hipStream_t stream, const std::vector<ItemSpec>& items, const Arena& in, size_t first,
              size_t count, uint32_t form, uint32_t element, uint32_t nulls, Call& c)
{
  std::vector<size_t> lens;
  for (size_t i = first; i < first + count; ++i)
    lens.push_back(items[i].capacity * element);
  c.out.plan(lens, kGuard, 0); // (256-byte aligned: every element type's alignment)
  std::vector<const uint8_t*> ptrs;
  std::vector<size_t> bytes, wanted, caps;
  std::vector<uint32_t> widths, match;
  std::vector<void*> outs;
  for (size_t i = 0; i < count; ++i) {
    const ItemSpec& it = items[first + i];
    ptrs.push_back(in.dev + in.at[first + i]);
    bytes.push_back(it.data.size());
    widths.push_back(it.bit_width);
    wanted.push_back(it.wanted);
    caps.push_back(it.capacity);
    match.push_back(it.match);
    outs.push_back(c.out.dev + c.out.at[i]);
  }
  const uint8_t** d_ptrs = device_copy(ptrs);
  size_t *d_bytes = device_copy(bytes), *d_wanted = device_copy(wanted), *d_caps = device_copy(caps);
  uint32_t *d_widths = device_copy(widths), *d_match = device_copy(match);
  void** d_outs = device_copy(outs);
  size_t *d_consumed = device_array<size_t>(count), *d_matches = device_array<size_t>(count);
  hipcompStatus_t* d_statuses = device_array<hipcompStatus_t>(count);
  HIP(hipMemset(d_consumed, kFill, (count ? count : 1) * sizeof(size_t)));
  HIP(hipMemset(d_matches, kFill, (count ? count : 1) * sizeof(size_t)));
  HIP(hipMemset(d_statuses, kFill, (count ? count : 1) * sizeof(hipcompStatus_t)));
  const bool no_widths = nulls == 3 && form == 2;
  m.decode_parquet_hybrid(d_ptrs, d_bytes, no_widths ? nullptr : d_widths, d_wanted, d_outs, d_caps, (nulls & 1) ? nullptr : d_consumed,
                          (nulls & 2) ? nullptr : d_match, (nulls & 2) ? nullptr : d_matches, d_statuses, count, (ParquetHybridForm)form,
                          type_of(element));
  HIP(hipStreamSynchronize(stream));
  c.r.statuses = host_copy(d_statuses, count);
  c.r.consumed = host_copy(d_consumed, count);
  c.r.matches = host_copy(d_matches, count);
  c.r.out = host_copy(c.out.dev, c.out.bytes);
  for (void* p : {(void*)d_ptrs, (void*)d_bytes, (void*)d_wanted, (void*)d_caps, (void*)d_widths, (void*)d_match, (void*)d_outs,
                  (void*)d_consumed, (void*)d_matches, (void*)d_statuses})
    HIP(hipFree(p));
}

struct CaseSpec
{
  uint32_t form = 0, element = 4, align = 0, nulls = 0, ones = 0;
  std::string outfile;
  std::vector<ItemSpec> items;
};

std::vector<CaseSpec> read_cases(const char* path)
{
  std::ifstream list(path);
  if (!list) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(3);
  }
  std::vector<CaseSpec> cases;
  std::string word;
  while (list >> word) {
    CaseSpec c;
    size_t n = 0;
    if (word != "case" || !(list >> c.form >> c.element >> c.align >> c.nulls >> c.ones >> c.outfile >> n)) {
      std::fprintf(stderr, "bad case line\n");
      std::exit(3);
    }
    for (size_t i = 0; i < n; ++i) {
      std::string file;
      uint64_t offset, length;
      ItemSpec it;
      if (!(list >> file >> offset >> length >> it.bit_width >> it.wanted >> it.capacity >> it.match)) {
        std::fprintf(stderr, "bad item line\n");
        std::exit(3);
      }
      it.data = slice_of(file, offset, length);
      c.items.push_back(std::move(it));
    }
    cases.push_back(std::move(c));
  }
  return cases;
}

void place_streams(const std::vector<ItemSpec>& items, size_t align, Arena& in)
{
  std::vector<size_t> lens;
  for (const ItemSpec& it : items)
    lens.push_back(it.data.size());
  in.plan(lens, kGuard, align);
  for (size_t i = 0; i < items.size(); ++i)
    if (!items[i].data.empty())
      HIP(hipMemcpy(in.dev + in.at[i], items[i].data.data(), items[i].data.size(), hipMemcpyHostToDevice));
}

int run_batch(const char* list)
{
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  for (const CaseSpec& c : read_cases(list)) {
    hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
    Arena in;
    place_streams(c.items, c.align, in);
    const size_t n = c.items.size();
    Call all;
    run_call(m, stream, c.items, in, 0, n, c.form, c.element, c.nulls, all);
    std::ofstream out(c.outfile, std::ios::binary);
    for (size_t i = 0; i < n; ++i) {
      const ItemSpec& it = c.items[i];
      const bool ok = all.r.statuses[i] == hipcompSuccess;
      const size_t size = ok ? (size_t)it.wanted : 0, cap_bytes = (size_t)it.capacity * c.element;
      const uint8_t* const mine = all.r.out.data() + all.out.at[i];
      // (a capacity below the wanted count: the item is refused, nothing behind the capacity is the output's)
      const size_t written = std::min(size * c.element, cap_bytes);
      const bool guards = all_fill(mine - kGuard, kGuard) && all_fill(mine + written, cap_bytes - written + kGuard);
      const bool untouched = all_fill(mine, cap_bytes);
      int one_status = -1, eq_one = -1;
      size_t one_consumed = 0, one_matches = 0;
      if (c.ones) {
        Call one;
        run_call(m, stream, c.items, in, i, 1, c.form, c.element, c.nulls, one);
        one_status = (int)one.r.statuses[0];
        one_consumed = one.r.consumed[0];
        one_matches = one.r.matches[0];
        eq_one = std::memcmp(one.r.out.data() + one.out.at[0] - kGuard, mine - kGuard, cap_bytes + 2 * kGuard) == 0;
      }
      std::printf("item %zu status %d consumed %zu matches %zu size %zu guards %d untouched %d one_status %d one_consumed %zu "
                  "one_matches %zu eq_one %d\n",
                  i, (int)all.r.statuses[i], (c.nulls & 1) ? 0 : all.r.consumed[i], (c.nulls & 2) ? 0 : all.r.matches[i], size,
                  (int)guards, (int)untouched, one_status, (c.nulls & 1) ? 0 : one_consumed, (c.nulls & 2) ? 0 : one_matches, eq_one);
      out.write(reinterpret_cast<const char*>(mine), (std::streamsize)written);
    }
    std::printf("case %zu\n", n);
    std::fflush(stdout);
  }
  HIP(hipStreamDestroy(stream));
  return 0;
}

// ---- the chained use ---------------------------------------------------------------------------------------------------
int run_chain(const char* list, const char* outfile)
{
  struct PageSpec
  {
    std::vector<uint8_t> levels, indices;
    uint32_t form, element;
    uint64_t rows;
  };
  std::vector<PageSpec> pages;
  std::ifstream f(list);
  std::string file;
  uint64_t lo, ll, io, il;
  PageSpec p;
  while (f >> file >> lo >> ll >> p.form >> io >> il >> p.element >> p.rows) {
    p.levels = slice_of(file, lo, ll);
    p.indices = slice_of(file, io, il);
    pages.push_back(p);
  }
  if (pages.empty())
    return 3;
  const size_t n = pages.size();
  const uint32_t form = pages[0].form, element = pages[0].element;
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
  Arena in_levels, in_indices, out_levels, out_indices;
  std::vector<size_t> a, b, c, d;
  for (const PageSpec& q : pages) {
    if (q.form != form || q.element != element)
      return 3; // (a call has one form and one element type)
    a.push_back(q.levels.size());
    b.push_back(q.indices.size());
    c.push_back(q.rows);
    d.push_back(q.rows * element);
  }
  in_levels.plan(a, kGuard, 0);
  in_indices.plan(b, kGuard, 0);
  out_levels.plan(c, kGuard, 0);
  out_indices.plan(d, kGuard, 0);
  std::vector<const uint8_t*> lp, ip;
  std::vector<void*> lo_ptrs, io_ptrs;
  std::vector<size_t> rows;
  for (size_t i = 0; i < n; ++i) {
    HIP(hipMemcpy(in_levels.dev + in_levels.at[i], pages[i].levels.data(), pages[i].levels.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(in_indices.dev + in_indices.at[i], pages[i].indices.data(), pages[i].indices.size(), hipMemcpyHostToDevice));
    lp.push_back(in_levels.dev + in_levels.at[i]);
    ip.push_back(in_indices.dev + in_indices.at[i]);
    lo_ptrs.push_back(out_levels.dev + out_levels.at[i]);
    io_ptrs.push_back(out_indices.dev + out_indices.at[i]);
    rows.push_back(pages[i].rows);
  }
  const uint8_t **d_lp = device_copy(lp), **d_ip = device_copy(ip);
  void **d_lo = device_copy(lo_ptrs), **d_io = device_copy(io_ptrs);
  size_t *d_lbytes = device_copy(a), *d_ibytes = device_copy(b), *d_rows = device_copy(rows);
  uint32_t *d_widths = device_copy(std::vector<uint32_t>(n, 1)), *d_ones = device_copy(std::vector<uint32_t>(n, 1));
  size_t *d_non_null = device_array<size_t>(n), *d_consumed = device_array<size_t>(n);
  hipcompStatus_t *d_ls = device_array<hipcompStatus_t>(n), *d_is = device_array<hipcompStatus_t>(n);
  // the levels and how many of them are the maximum level; then the indices, as many as that: the count never
  // leaves the device, and nothing waits between the two calls
  m.decode_parquet_hybrid(d_lp, d_lbytes, d_widths, d_rows, d_lo, d_rows, nullptr, d_ones, d_non_null, d_ls, n, (ParquetHybridForm)form,
                          HIPCOMP_TYPE_UCHAR);
  m.decode_parquet_hybrid(d_ip, d_ibytes, nullptr, d_non_null, d_io, d_rows, d_consumed, nullptr, nullptr, d_is, n,
                          ParquetHybridForm::WidthPrefixed, type_of(element));
  HIP(hipStreamSynchronize(stream));
  const auto ls = host_copy(d_ls, n), is = host_copy(d_is, n);
  const auto non_null = host_copy(d_non_null, n), consumed = host_copy(d_consumed, n);
  const auto lv = host_copy(out_levels.dev, out_levels.bytes), iv = host_copy(out_indices.dev, out_indices.bytes);
  std::ofstream out(outfile, std::ios::binary);
  for (size_t i = 0; i < n; ++i) {
    std::printf("page %zu levels_status %d index_status %d non_null %zu index_consumed %zu\n", i, (int)ls[i], (int)is[i], non_null[i],
                consumed[i]);
    out.write(reinterpret_cast<const char*>(lv.data() + out_levels.at[i]), (std::streamsize)pages[i].rows);
    out.write(reinterpret_cast<const char*>(iv.data() + out_indices.at[i]), (std::streamsize)(std::min<size_t>(non_null[i], pages[i].rows) * element));
  }
  HIP(hipStreamDestroy(stream));
  return 0;
}

// ---- misuse ----------------------------------------------------------------------------------------------------------
int run_misuse()
{
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
  const std::vector<uint8_t> bytes = {0x04, 0x01}; // 2 x 1
  const uint8_t* d_stream = device_copy(bytes);
  uint8_t* d_out = device_array<uint8_t>(16);
  HIP(hipMemset(d_out, kFill, 16));
  const uint8_t** d_ptrs = device_copy(std::vector<const uint8_t*>{d_stream});
  void** d_outs = device_copy(std::vector<void*>{d_out});
  size_t *d_bytes = device_copy(std::vector<size_t>{2}), *d_wanted = device_copy(std::vector<size_t>{2}), *d_caps = device_copy(std::vector<size_t>{2});
  uint32_t *d_widths = device_copy(std::vector<uint32_t>{1}), *d_match = device_copy(std::vector<uint32_t>{1});
  size_t *d_consumed = device_array<size_t>(1), *d_matches = device_array<size_t>(1);
  hipcompStatus_t* d_status = device_array<hipcompStatus_t>(1);
  HIP(hipMemset(d_status, kFill, sizeof(hipcompStatus_t)));
  int threw = 0, quiet = 0;
  auto attempt = [&](const uint8_t* const* ptrs, const size_t* nbytes, const uint32_t* widths, const size_t* wanted, void* const* outs,
                     const size_t* caps, const uint32_t* match, size_t* matches, hipcompStatus_t* statuses, size_t items,
                     ParquetHybridForm form, hipcompType_t type) {
    try {
      m.decode_parquet_hybrid(ptrs, nbytes, widths, wanted, outs, caps, d_consumed, match, matches, statuses, items, form, type);
      ++quiet;
    } catch (const std::runtime_error&) {
      ++threw;
    }
  };
  const ParquetHybridForm bare = ParquetHybridForm::Bare;
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, (size_t(1) << 20) + 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(nullptr, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, nullptr, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, nullptr, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, nullptr, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, ParquetHybridForm::LengthPrefixed, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, d_widths, nullptr, d_outs, d_caps, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, nullptr, d_caps, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, nullptr, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, nullptr, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, nullptr, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, nullptr, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  for (hipcompType_t t : {HIPCOMP_TYPE_CHAR, HIPCOMP_TYPE_SHORT, HIPCOMP_TYPE_INT, HIPCOMP_TYPE_ULONGLONG, HIPCOMP_TYPE_BITS})
    attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, bare, t);
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, (ParquetHybridForm)3, HIPCOMP_TYPE_UCHAR);
  const int threw_all = threw;
  HIP(hipStreamSynchronize(stream));
  // nothing was launched by any of them
  const bool nothing = all_fill(host_copy(d_out, 16).data(), 16)
                       && all_fill(reinterpret_cast<const uint8_t*>(host_copy(d_status, 1).data()), sizeof(hipcompStatus_t));
  // no items: nothing to do, whatever the arrays
  attempt(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, bare, HIPCOMP_TYPE_UINT);
  // and the call as it is meant
  attempt(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_match, d_matches, d_status, 1, bare, HIPCOMP_TYPE_UCHAR);
  HIP(hipStreamSynchronize(stream));
  const auto out = host_copy(d_out, 16);
  const bool decoded = out[0] == 1 && out[1] == 1 && all_fill(out.data() + 2, 14) && host_copy(d_status, 1)[0] == hipcompSuccess
                       && host_copy(d_matches, 1)[0] == 2 && host_copy(d_consumed, 1)[0] == 2;
  std::printf("threw %d quiet %d nothing_launched %d decoded %d\n", threw_all, quiet, (int)nothing, (int)decoded);
  HIP(hipStreamDestroy(stream));
  return 0;
}

// ---- timing ------------------------------------------------------------------------------------------------------------
#ifdef HYBRID_HOST_DECODER
float median(std::vector<float> v)
{
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

template <class T>
void host_decode(const std::vector<ItemSpec>& items, const std::vector<uint8_t>& in, const Arena& a, uint32_t form, std::vector<T>& out,
                 const std::vector<size_t>& out_at)
{
  for (size_t i = 0; i < items.size(); ++i) {
    uint64_t matches = 0;
    (void)hcamd::pqh::decode_item(in.data() + a.at[i], items[i].data.size(), form, items[i].bit_width, items[i].wanted, items[i].capacity,
                                  out.data() + out_at[i], items[i].match, matches);
  }
}

template <class T>
int time_as(const CaseSpec& c, int reps)
{
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
  Arena in;
  place_streams(c.items, 0, in);
  const size_t n = c.items.size();
  std::vector<size_t> out_at, bytes, wanted, caps;
  std::vector<uint32_t> widths, match;
  size_t total = 0, in_bytes = 0;
  for (const ItemSpec& it : c.items) {
    out_at.push_back(total);
    total += round_up((size_t)it.capacity, 64);
    in_bytes += it.data.size();
    bytes.push_back(it.data.size());
    wanted.push_back(it.wanted);
    caps.push_back(it.capacity);
    widths.push_back(it.bit_width);
    match.push_back(it.match);
  }
  T *d_out = device_array<T>(total), *d_twin = device_array<T>(total);
  std::vector<const uint8_t*> ptrs;
  std::vector<void*> outs;
  for (size_t i = 0; i < n; ++i) {
    ptrs.push_back(in.dev + in.at[i]);
    outs.push_back(d_out + out_at[i]);
  }
  const uint8_t** d_ptrs = device_copy(ptrs);
  void** d_outs = device_copy(outs);
  size_t *d_bytes = device_copy(bytes), *d_wanted = device_copy(wanted), *d_caps = device_copy(caps);
  uint32_t *d_widths = device_copy(widths), *d_match = device_copy(match);
  size_t *d_consumed = device_array<size_t>(n), *d_matches = device_array<size_t>(n);
  hipcompStatus_t* d_statuses = device_array<hipcompStatus_t>(n);
  std::vector<uint8_t> h_in(in.bytes);
  std::vector<T> h_out(total);
  hipEvent_t e0, e1;
  HIP(hipEventCreate(&e0));
  HIP(hipEventCreate(&e1));
  std::vector<float> t_call, t_copy, t_host;
  for (int r = -2; r < reps; ++r) { // (two unrecorded turns first)
    float ms;
    HIP(hipEventRecord(e0, stream));
    m.decode_parquet_hybrid(d_ptrs, d_bytes, d_widths, d_wanted, d_outs, d_caps, d_consumed, d_match, d_matches, d_statuses, n,
                            (ParquetHybridForm)c.form, type_of(sizeof(T)));
    HIP(hipEventRecord(e1, stream));
    HIP(hipEventSynchronize(e1));
    HIP(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0)
      t_call.push_back(ms);
    HIP(hipEventRecord(e0, stream));
    HIP(hipMemcpyAsync(d_twin, d_out, total * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIP(hipEventRecord(e1, stream));
    HIP(hipEventSynchronize(e1));
    HIP(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0)
      t_copy.push_back(ms);
    HIP(hipEventRecord(e0, stream));
    HIP(hipMemcpyAsync(h_in.data(), in.dev, in.bytes, hipMemcpyDeviceToHost, stream));
    HIP(hipStreamSynchronize(stream));
    host_decode(c.items, h_in, in, c.form, h_out, out_at);
    HIP(hipMemcpyAsync(d_twin, h_out.data(), total * sizeof(T), hipMemcpyHostToDevice, stream));
    HIP(hipEventRecord(e1, stream));
    HIP(hipEventSynchronize(e1));
    HIP(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0)
      t_host.push_back(ms);
  }
  // the two ways wrote the same values
  const auto a = host_copy(d_out, total), b = host_copy(d_twin, total);
  const auto statuses = host_copy(d_statuses, n);
  bool same = true;
  size_t values = 0;
  for (size_t i = 0; i < n; ++i) {
    same = same && statuses[i] == hipcompSuccess && std::memcmp(a.data() + out_at[i], b.data() + out_at[i], c.items[i].wanted * sizeof(T)) == 0;
    values += c.items[i].wanted;
  }
  std::printf("items %zu values %zu stream_bytes %zu out_bytes %zu same %d call_ms %.4f copy_ms %.4f host_ms %.4f reps %d\n", n, values,
              in_bytes, total * sizeof(T), (int)same, median(t_call), median(t_copy), median(t_host), reps);
  HIP(hipStreamDestroy(stream));
  return same ? 0 : 4;
}

int run_time(const char* list, int reps)
{
  const std::vector<CaseSpec> cases = read_cases(list);
  if (cases.size() != 1 || reps < 1)
    return 3;
  const CaseSpec& c = cases[0];
  return c.element == 1 ? time_as<uint8_t>(c, reps) : c.element == 2 ? time_as<uint16_t>(c, reps) : time_as<uint32_t>(c, reps);
}
#endif

} // namespace

int main(int argc, char** argv)
{
  try {
    if (argc == 3 && std::string(argv[1]) == "batch")
      return run_batch(argv[2]);
    if (argc == 4 && std::string(argv[1]) == "chain")
      return run_chain(argv[2], argv[3]);
    if (argc == 2 && std::string(argv[1]) == "misuse")
      return run_misuse();
#ifdef HYBRID_HOST_DECODER
    if (argc == 4 && std::string(argv[1]) == "time")
      return run_time(argv[2], std::atoi(argv[3]));
#endif
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 6;
  }
  std::fprintf(stderr, "usage: %s batch LIST | chain LIST OUT | misuse | time LIST REPS\n", argv[0]);
  return 2;
}
