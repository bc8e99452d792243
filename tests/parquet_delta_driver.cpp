// Batches of Parquet DELTA_BINARY_PACKED streams in one call (hipcomp/cascaded.hpp: decode_parquet_delta of the Cascaded
// manager) driven on a GPU for tests/test_parquet_delta_gpu.py and scripts/quick_parquet_delta.py.  Written against
// include/ and linked to libhipcomp.so.
//
//   batch LIST     LIST holds cases: a line "case OUTPUT ELEMENT ALIGN NULLS COUNTED ONES OUTFILE N" and N lines
//                  "FILE OFFSET LENGTH WANTED CAPACITY".  OUTPUT 0 | 1 (ParquetDeltaOutput); ELEMENT 4 | 8 bytes; ALIGN: every
//                  stream lies ALIGN bytes behind a 256-byte aligned address; NULLS: 1 device_value_counts is null, 2
//                  device_consumed_bytes is, 3 both; COUNTED 0: device_num_values is null; ONES 1: every item is also decoded
//                  as a batch of its own, into a twin of its output.
//                  Per item a line "item I status .. consumed .. count .. guards G untouched U one_status .. one_consumed ..
//                  one_count .. eq_one E".  guards: the 64 bytes on both sides of the output's CAPACITY elements are as they
//                  were.  untouched: so is the whole output.  OUTFILE takes, item by item, the CAPACITY elements.
//   chain LIST OUT OUTPUT ELEMENT   the chained use: lines "FILE LEVELS_OFFSET LEVELS_LENGTH FORM VALUES_OFFSET VALUES_LENGTH
//                  ROWS", a page each.  decode_parquet_hybrid decodes the definition levels (width 1) of all pages and counts
//                  the ones; decode_parquet_delta takes that device array as its device_num_values; nothing is copied to the
//                  host or synchronised between the two.  Per page "page I levels_status .. values_status .. non_null ..
//                  count .. consumed ..", OUT takes per page the ROWS levels and the ROWS + 1 elements of the output.
//   misuse         what throws before a launch
//   time LIST REPS one case line and its items: REPS alternating timings (HIP events) of the one call, of a device-to-device
//                  copy of as many bytes as it writes, and of today's way: the streams copied to the host, decoded there by
//                  one thread (the plan header's decoder), the elements copied back
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
#ifdef DELTA_HOST_DECODER
#include "parquet_delta_plan.hpp"
#endif

using hipcomp::ParquetDeltaOutput;
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

hipcompType_t type_of(uint32_t element) { return element == 4 ? HIPCOMP_TYPE_INT : HIPCOMP_TYPE_LONGLONG; }

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
  uint64_t wanted = 0, capacity = 0;
};

struct Result
{
  std::vector<hipcompStatus_t> statuses;
  std::vector<size_t> consumed, counts;
  std::vector<uint8_t> out; // the output arena, whole
};

struct CaseSpec
{
  uint32_t output = 0, element = 8, align = 0, nulls = 0, counted = 0, ones = 0;
  std::string outfile;
  std::vector<ItemSpec> items;
};

// one call over items [first, first + count) of the case; the streams lie in `in`, the outputs in a fresh arena
struct Call
{
  Arena out;
  Result r;
};
void run_call(hipcomp::CascadedManager& m, hipStream_t stream, const CaseSpec& c, const Arena& in, size_t first, size_t count, Call& call)
{
  std::vector<size_t> lens;
  for (size_t i = first; i < first + count; ++i)
    lens.push_back(c.items[i].capacity * c.element);
  call.out.plan(lens, kGuard, 0); // (256-byte aligned: every element type's alignment)
  std::vector<const uint8_t*> ptrs;
  std::vector<size_t> bytes, wanted, caps;
  std::vector<void*> outs;
  for (size_t i = 0; i < count; ++i) {
    const ItemSpec& it = c.items[first + i];
    ptrs.push_back(in.dev + in.at[first + i]);
    bytes.push_back(it.data.size());
    wanted.push_back(it.wanted);
    caps.push_back(it.capacity);
    outs.push_back(call.out.dev + call.out.at[i]);
  }
  const uint8_t** d_ptrs = device_copy(ptrs);
  size_t *d_bytes = device_copy(bytes), *d_wanted = device_copy(wanted), *d_caps = device_copy(caps);
  void** d_outs = device_copy(outs);
  size_t *d_consumed = device_array<size_t>(count), *d_counts = device_array<size_t>(count);
  hipcompStatus_t* d_statuses = device_array<hipcompStatus_t>(count);
  HIP(hipMemset(d_consumed, kFill, (count ? count : 1) * sizeof(size_t)));
  HIP(hipMemset(d_counts, kFill, (count ? count : 1) * sizeof(size_t)));
  HIP(hipMemset(d_statuses, kFill, (count ? count : 1) * sizeof(hipcompStatus_t)));
  m.decode_parquet_delta(d_ptrs, d_bytes, c.counted ? d_wanted : nullptr, d_outs, d_caps, (c.nulls & 1) ? nullptr : d_counts,
                         (c.nulls & 2) ? nullptr : d_consumed, d_statuses, count, (ParquetDeltaOutput)c.output, type_of(c.element));
  HIP(hipStreamSynchronize(stream));
  call.r.statuses = host_copy(d_statuses, count);
  call.r.consumed = host_copy(d_consumed, count);
  call.r.counts = host_copy(d_counts, count);
  call.r.out = host_copy(call.out.dev, call.out.bytes);
  for (void* p : {(void*)d_ptrs, (void*)d_bytes, (void*)d_wanted, (void*)d_caps, (void*)d_outs, (void*)d_consumed, (void*)d_counts,
                  (void*)d_statuses})
    HIP(hipFree(p));
}

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
    if (word != "case" || !(list >> c.output >> c.element >> c.align >> c.nulls >> c.counted >> c.ones >> c.outfile >> n)
        || (c.element != 4 && c.element != 8)) {
      std::fprintf(stderr, "bad case line\n");
      std::exit(3);
    }
    for (size_t i = 0; i < n; ++i) {
      std::string file;
      uint64_t offset, length;
      ItemSpec it;
      if (!(list >> file >> offset >> length >> it.wanted >> it.capacity)) {
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
    run_call(m, stream, c, in, 0, n, all);
    std::ofstream out(c.outfile, std::ios::binary);
    for (size_t i = 0; i < n; ++i) {
      const size_t cap_bytes = (size_t)c.items[i].capacity * c.element;
      const uint8_t* const mine = all.r.out.data() + all.out.at[i];
      const bool guards = all_fill(mine - kGuard, kGuard) && all_fill(mine + cap_bytes, kGuard);
      const bool untouched = all_fill(mine, cap_bytes);
      int one_status = -1, eq_one = -1;
      size_t one_consumed = 0, one_count = 0;
      if (c.ones) {
        Call one;
        run_call(m, stream, c, in, i, 1, one);
        one_status = (int)one.r.statuses[0];
        one_consumed = one.r.consumed[0];
        one_count = one.r.counts[0];
        eq_one = std::memcmp(one.r.out.data() + one.out.at[0] - kGuard, mine - kGuard, cap_bytes + 2 * kGuard) == 0;
      }
      std::printf("item %zu status %d consumed %zu count %zu guards %d untouched %d one_status %d one_consumed %zu one_count %zu "
                  "eq_one %d\n",
                  i, (int)all.r.statuses[i], (c.nulls & 2) ? 0 : all.r.consumed[i], (c.nulls & 1) ? 0 : all.r.counts[i], (int)guards,
                  (int)untouched, one_status, (c.nulls & 2) ? 0 : one_consumed, (c.nulls & 1) ? 0 : one_count, eq_one);
      out.write(reinterpret_cast<const char*>(mine), (std::streamsize)cap_bytes);
    }
    std::printf("case %zu\n", n);
    std::fflush(stdout);
  }
  HIP(hipStreamDestroy(stream));
  return 0;
}

// ---- the chained use ---------------------------------------------------------------------------------------------------
int run_chain(const char* list, const char* outfile, uint32_t output, uint32_t element)
{
  struct PageSpec
  {
    std::vector<uint8_t> levels, values;
    uint32_t form;
    uint64_t rows;
  };
  std::vector<PageSpec> pages;
  std::ifstream f(list);
  std::string file;
  uint64_t lo, ll, vo, vl;
  PageSpec p;
  while (f >> file >> lo >> ll >> p.form >> vo >> vl >> p.rows) {
    p.levels = slice_of(file, lo, ll);
    p.values = slice_of(file, vo, vl);
    pages.push_back(p);
  }
  if (pages.empty() || (element != 4 && element != 8))
    return 3;
  const size_t n = pages.size();
  const uint32_t form = pages[0].form;
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  hipcomp::CascadedManager m(hipcompBatchedCascadedDefaultOpts, stream, 0);
  Arena in_levels, in_values, out_levels, out_values;
  std::vector<size_t> a, b, c, d, rows, caps;
  for (const PageSpec& q : pages) {
    if (q.form != form)
      return 3; // (a call has one form)
    a.push_back(q.levels.size());
    b.push_back(q.values.size());
    c.push_back(q.rows);
    d.push_back((q.rows + 1) * element);
    rows.push_back(q.rows);
    caps.push_back(q.rows + 1);
  }
  in_levels.plan(a, kGuard, 0);
  in_values.plan(b, kGuard, 0);
  out_levels.plan(c, kGuard, 0);
  out_values.plan(d, kGuard, 0);
  std::vector<const uint8_t*> lp, vp;
  std::vector<void*> lo_ptrs, vo_ptrs;
  for (size_t i = 0; i < n; ++i) {
    HIP(hipMemcpy(in_levels.dev + in_levels.at[i], pages[i].levels.data(), pages[i].levels.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(in_values.dev + in_values.at[i], pages[i].values.data(), pages[i].values.size(), hipMemcpyHostToDevice));
    lp.push_back(in_levels.dev + in_levels.at[i]);
    vp.push_back(in_values.dev + in_values.at[i]);
    lo_ptrs.push_back(out_levels.dev + out_levels.at[i]);
    vo_ptrs.push_back(out_values.dev + out_values.at[i]);
  }
  const uint8_t **d_lp = device_copy(lp), **d_vp = device_copy(vp);
  void **d_lo = device_copy(lo_ptrs), **d_vo = device_copy(vo_ptrs);
  size_t *d_lbytes = device_copy(a), *d_vbytes = device_copy(b), *d_rows = device_copy(rows), *d_caps = device_copy(caps);
  uint32_t *d_widths = device_copy(std::vector<uint32_t>(n, 1)), *d_ones = device_copy(std::vector<uint32_t>(n, 1));
  size_t *d_non_null = device_array<size_t>(n), *d_counts = device_array<size_t>(n), *d_consumed = device_array<size_t>(n);
  hipcompStatus_t *d_ls = device_array<hipcompStatus_t>(n), *d_vs = device_array<hipcompStatus_t>(n);
  // the levels and how many of them are the maximum level; then the values, as many as that: the count never leaves
  // the device, and nothing waits between the two calls
  m.decode_parquet_hybrid(d_lp, d_lbytes, d_widths, d_rows, d_lo, d_rows, nullptr, d_ones, d_non_null, d_ls, n, (ParquetHybridForm)form,
                          HIPCOMP_TYPE_UCHAR);
  m.decode_parquet_delta(d_vp, d_vbytes, d_non_null, d_vo, d_caps, d_counts, d_consumed, d_vs, n, (ParquetDeltaOutput)output,
                         type_of(element));
  HIP(hipStreamSynchronize(stream));
  const auto ls = host_copy(d_ls, n), vs = host_copy(d_vs, n);
  const auto non_null = host_copy(d_non_null, n), counts = host_copy(d_counts, n), consumed = host_copy(d_consumed, n);
  const auto lv = host_copy(out_levels.dev, out_levels.bytes), vv = host_copy(out_values.dev, out_values.bytes);
  std::ofstream out(outfile, std::ios::binary);
  for (size_t i = 0; i < n; ++i) {
    std::printf("page %zu levels_status %d values_status %d non_null %zu count %zu consumed %zu\n", i, (int)ls[i], (int)vs[i], non_null[i],
                counts[i], consumed[i]);
    out.write(reinterpret_cast<const char*>(lv.data() + out_levels.at[i]), (std::streamsize)pages[i].rows);
    out.write(reinterpret_cast<const char*>(vv.data() + out_values.at[i]), (std::streamsize)((pages[i].rows + 1) * element));
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
  // block 128, 4 miniblocks, 2 values, first 7; minimum delta -3, widths 0 x 4: 7 and 4
  const std::vector<uint8_t> bytes = {0x80, 0x01, 0x04, 0x02, 0x0E, 0x05, 0x00, 0x00, 0x00, 0x00};
  const uint8_t* d_stream = device_copy(bytes);
  int32_t* d_out = device_array<int32_t>(4);
  HIP(hipMemset(d_out, kFill, 16));
  const uint8_t** d_ptrs = device_copy(std::vector<const uint8_t*>{d_stream});
  void** d_outs = device_copy(std::vector<void*>{d_out});
  size_t *d_bytes = device_copy(std::vector<size_t>{bytes.size()}), *d_wanted = device_copy(std::vector<size_t>{2}),
         *d_caps = device_copy(std::vector<size_t>{2});
  size_t *d_consumed = device_array<size_t>(1), *d_counts = device_array<size_t>(1);
  hipcompStatus_t* d_status = device_array<hipcompStatus_t>(1);
  HIP(hipMemset(d_status, kFill, sizeof(hipcompStatus_t)));
  int threw = 0, quiet = 0;
  auto attempt = [&](const uint8_t* const* ptrs, const size_t* nbytes, void* const* outs, const size_t* caps, hipcompStatus_t* statuses,
                     size_t items, ParquetDeltaOutput output, hipcompType_t type) {
    try {
      m.decode_parquet_delta(ptrs, nbytes, d_wanted, outs, caps, d_counts, d_consumed, statuses, items, output, type);
      ++quiet;
    } catch (const std::runtime_error&) {
      ++threw;
    }
  };
  const ParquetDeltaOutput values = ParquetDeltaOutput::Values;
  attempt(d_ptrs, d_bytes, d_outs, d_caps, d_status, (size_t(1) << 20) + 1, values, HIPCOMP_TYPE_INT);
  attempt(nullptr, d_bytes, d_outs, d_caps, d_status, 1, values, HIPCOMP_TYPE_INT);
  attempt(d_ptrs, nullptr, d_outs, d_caps, d_status, 1, values, HIPCOMP_TYPE_INT);
  attempt(d_ptrs, d_bytes, nullptr, d_caps, d_status, 1, values, HIPCOMP_TYPE_INT);
  attempt(d_ptrs, d_bytes, d_outs, nullptr, d_status, 1, values, HIPCOMP_TYPE_INT);
  attempt(d_ptrs, d_bytes, d_outs, d_caps, nullptr, 1, values, HIPCOMP_TYPE_INT);
  for (hipcompType_t t : {HIPCOMP_TYPE_CHAR, HIPCOMP_TYPE_UCHAR, HIPCOMP_TYPE_SHORT, HIPCOMP_TYPE_USHORT, HIPCOMP_TYPE_UINT,
                          HIPCOMP_TYPE_ULONGLONG, HIPCOMP_TYPE_BITS})
    attempt(d_ptrs, d_bytes, d_outs, d_caps, d_status, 1, values, t);
  attempt(d_ptrs, d_bytes, d_outs, d_caps, d_status, 1, (ParquetDeltaOutput)2, HIPCOMP_TYPE_INT);
  const int threw_all = threw;
  HIP(hipStreamSynchronize(stream));
  // nothing was launched by any of them
  const bool nothing = all_fill(reinterpret_cast<const uint8_t*>(host_copy(d_out, 4).data()), 16)
                       && all_fill(reinterpret_cast<const uint8_t*>(host_copy(d_status, 1).data()), sizeof(hipcompStatus_t));
  // no items: nothing to do, whatever the arrays
  attempt(nullptr, nullptr, nullptr, nullptr, nullptr, 0, values, HIPCOMP_TYPE_LONGLONG);
  // and the call as it is meant
  attempt(d_ptrs, d_bytes, d_outs, d_caps, d_status, 1, values, HIPCOMP_TYPE_INT);
  HIP(hipStreamSynchronize(stream));
  const auto out = host_copy(d_out, 4);
  const bool decoded = out[0] == 7 && out[1] == 4 && all_fill(reinterpret_cast<const uint8_t*>(out.data() + 2), 8)
                       && host_copy(d_status, 1)[0] == hipcompSuccess && host_copy(d_counts, 1)[0] == 2 && host_copy(d_consumed, 1)[0] == 10;
  std::printf("threw %d quiet %d nothing_launched %d decoded %d\n", threw_all, quiet, (int)nothing, (int)decoded);
  HIP(hipStreamDestroy(stream));
  return 0;
}

// ---- timing ------------------------------------------------------------------------------------------------------------
#ifdef DELTA_HOST_DECODER
float median(std::vector<float> v)
{
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
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
  size_t total = 0, in_bytes = 0;
  for (const ItemSpec& it : c.items) {
    out_at.push_back(total);
    total += round_up((size_t)it.capacity, 64);
    in_bytes += it.data.size();
    bytes.push_back(it.data.size());
    wanted.push_back(it.wanted);
    caps.push_back(it.capacity);
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
  size_t *d_consumed = device_array<size_t>(n), *d_counts = device_array<size_t>(n);
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
    m.decode_parquet_delta(d_ptrs, d_bytes, d_wanted, d_outs, d_caps, d_counts, d_consumed, d_statuses, n, (ParquetDeltaOutput)c.output,
                           type_of(sizeof(T)));
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
    for (size_t i = 0; i < n; ++i)
      (void)hcamd::pqd::decode_item(h_in.data() + in.at[i], c.items[i].data.size(), true, c.items[i].wanted, c.items[i].capacity, c.output,
                                    h_out.data() + out_at[i]);
    HIP(hipMemcpyAsync(d_twin, h_out.data(), total * sizeof(T), hipMemcpyHostToDevice, stream));
    HIP(hipEventRecord(e1, stream));
    HIP(hipEventSynchronize(e1));
    HIP(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0)
      t_host.push_back(ms);
  }
  // the two ways wrote the same elements
  const auto a = host_copy(d_out, total), b = host_copy(d_twin, total);
  const auto statuses = host_copy(d_statuses, n);
  bool same = true;
  size_t values = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t elements = c.items[i].wanted + (c.output == 1 ? 1 : 0);
    same = same && statuses[i] == hipcompSuccess && std::memcmp(a.data() + out_at[i], b.data() + out_at[i], elements * sizeof(T)) == 0;
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
  return cases[0].element == 4 ? time_as<uint32_t>(cases[0], reps) : time_as<uint64_t>(cases[0], reps);
}
#endif

} // namespace

int main(int argc, char** argv)
{
  try {
    if (argc == 3 && std::string(argv[1]) == "batch")
      return run_batch(argv[2]);
    if (argc == 6 && std::string(argv[1]) == "chain")
      return run_chain(argv[2], argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]));
    if (argc == 2 && std::string(argv[1]) == "misuse")
      return run_misuse();
#ifdef DELTA_HOST_DECODER
    if (argc == 4 && std::string(argv[1]) == "time")
      return run_time(argv[2], std::atoi(argv[3]));
#endif
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 6;
  }
  std::fprintf(stderr, "usage: %s batch LIST | chain LIST OUT OUTPUT ELEMENT | misuse | time LIST REPS\n", argv[0]);
  return 2;
}
