// The pages of Parquet column chunks in one call (hipcomp/snappy.hpp: decompress_parquet_pages, get_parquet_pages_sizes)
// driven on a GPU for tests/test_parquet_pages_gpu.py and scripts/quick_parquet_pages.py.  Written against include/ and
// linked to libhipcomp.so.
//
//   batch LIST     LIST holds cases: a line "case POLICY CODEC SCRATCH PASS_PAGES TABLES ALIGN ONES OUTFILE N" and N lines
//                  "FILE OFFSET LENGTH CAP ROWS".  SCRATCH own | caller (a caller's scratch buffer of
//                  get_required_scratch_buffer_size() bytes, guard bytes behind it).  PASS_PAGES: set_parquet_pass_pages.
//                  TABLES 0: device_page_ptrs is null.  ALIGN: every chunk and every output lies ALIGN bytes behind a
//                  256-byte aligned address.  CAP E | S | O: the output's capacity is what the size query says, one byte
//                  less, 77 more; ROWS E | S | O the same for the page table (one row less, 3 more).  ONES 1: every item is
//                  also read as a batch of its own, with the same buffers' twins.
//                  Per item a line "item I status .. size .. pages .. q_status .. q_size .. q_pages .. guards G untouched U
//                  one_status .. one_size .. one_pages .. eq_one E", then "case K scratch_intact B stats_pages .. passes ..
//                  pass_pages ..".  guards: the 64 bytes on both sides of the output and the row on both sides of the table
//                  are as they were.  untouched: so is the whole output.  OUTFILE takes, item by item, the `size` bytes of
//                  the output and the `pages` rows of the table.
//   misuse         what throws before a launch
//   time LIST REPS one case line and its items: REPS alternating timings (HIP events) of one decompress_parquet_pages against
//                  today's way -- the headers walked on the host from a host copy of the same chunks, the lists of the
//                  compressed parts copied to the device, one hipcompBatchedSnappyDecompressAsync over all of them (the
//                  chunks are V1 data pages under Snappy: there is nothing to copy)
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

#include "hipcomp/snappy.h"
#include "hipcomp/snappy.hpp"

using hipcomp::ParquetCodec;
using hipcomp::ParquetPageInfo;

#define HIP(x)                                                                                          \
  do {                                                                                                  \
    const hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) {                                                                             \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);                  \
      std::exit(5);                                                                                     \
    }                                                                                                   \
  } while (0)

namespace {

constexpr size_t kGuard = 64, kRow = sizeof(ParquetPageInfo);
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

struct ItemSpec
{
  std::vector<uint8_t> data;
  char cap = 'E', rows = 'E';
};

// An arena of buffers with guards around each: buffer i is [at[i], at[i] + len[i]) of the arena, `guard` bytes of
// fill on both sides, at[i] = `align` behind a multiple of 256 (`align` < 256) -- or, for tables, 8-byte aligned.
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

struct Buffers
{
  Arena outs, tables;
  std::vector<uint8_t> h_outs, h_tables;
  void plan(const std::vector<size_t>& caps, const std::vector<size_t>& rows, size_t align)
  {
    outs.plan(caps, kGuard, align);
    std::vector<size_t> table_bytes;
    for (size_t r : rows)
      table_bytes.push_back(r * kRow);
    tables.plan(table_bytes, kRow, 0);
  }
  void fetch()
  {
    h_outs = host_copy(outs.dev, outs.bytes);
    h_tables = host_copy(tables.dev, tables.bytes);
  }
  bool guards(size_t i) const
  {
    return all_fill(&h_outs[outs.at[i] - kGuard], kGuard) && all_fill(&h_outs[outs.at[i] + outs.len[i]], kGuard)
           && all_fill(&h_tables[tables.at[i] - kRow], kRow) && all_fill(&h_tables[tables.at[i] + tables.len[i]], kRow);
  }
  bool untouched(size_t i) const { return all_fill(&h_outs[outs.at[i]], outs.len[i]); }
};

struct Results
{
  std::vector<size_t> sizes, pages;
  std::vector<hipcompStatus_t> statuses;
};

struct Case
{
  int policy = 0, codec = 1, tables = 1, ones = 0;
  std::string scratch = "own", outfile;
  size_t pass_pages = 0, align = 0;
  std::vector<ItemSpec> items;
};

std::vector<Case> read_cases(const char* list)
{
  std::ifstream f(list);
  std::vector<Case> cases;
  std::string word;
  while (f >> word) {
    if (word != "case")
      std::exit(2);
    Case c;
    size_t n = 0;
    f >> c.policy >> c.codec >> c.scratch >> c.pass_pages >> c.tables >> c.align >> c.ones >> c.outfile >> n;
    for (size_t i = 0; i < n; ++i) {
      std::string file;
      uint64_t offset = 0, length = 0;
      ItemSpec it;
      f >> file >> offset >> length >> it.cap >> it.rows;
      it.data = slice_of(file, offset, length);
      c.items.push_back(std::move(it));
    }
    cases.push_back(std::move(c));
  }
  return cases;
}

size_t sized(char word, size_t exact, size_t more)
{
  return word == 'S' ? (exact ? exact - 1 : 0) : word == 'O' ? exact + more : exact;
}

int run_case(size_t number, const Case& c)
{
  const size_t n = c.items.size();
  const ParquetCodec codec = c.codec ? ParquetCodec::Snappy : ParquetCodec::Uncompressed;
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  int intact = 1;
  {
    hipcomp::SnappyManager m(65536, stream, 0, (hipcomp::ChecksumPolicy)c.policy);
    uint8_t* scratch = nullptr;
    size_t scratch_bytes = 0;
    if (c.scratch == "caller") {
      scratch_bytes = m.get_required_scratch_buffer_size();
      HIP(hipMalloc((void**)&scratch, scratch_bytes + kGuard));
      HIP(hipMemset(scratch + scratch_bytes, kFill, kGuard));
      m.set_scratch_buffer(scratch);
    }
    m.set_parquet_pass_pages(c.pass_pages);
    // the chunks
    Arena in;
    std::vector<size_t> lens;
    for (const ItemSpec& it : c.items)
      lens.push_back(it.data.size());
    in.plan(lens, kGuard, c.align);
    std::vector<const uint8_t*> chunk_ptrs;
    for (size_t i = 0; i < n; ++i) {
      if (lens[i])
        HIP(hipMemcpy(in.dev + in.at[i], c.items[i].data.data(), lens[i], hipMemcpyHostToDevice));
      chunk_ptrs.push_back(in.dev + in.at[i]);
    }
    const uint8_t** d_chunk_ptrs = device_copy(chunk_ptrs);
    size_t* d_chunk_bytes = device_copy(lens);
    // the size query
    size_t* d_q_pages = device_array<size_t>(n);
    size_t* d_q_sizes = device_array<size_t>(n);
    hipcompStatus_t* d_q_statuses = device_array<hipcompStatus_t>(n);
    m.get_parquet_pages_sizes(d_chunk_ptrs, d_chunk_bytes, d_q_pages, d_q_sizes, d_q_statuses, n, codec);
    HIP(hipStreamSynchronize(stream));
    const std::vector<size_t> q_pages = host_copy(d_q_pages, n), q_sizes = host_copy(d_q_sizes, n);
    const std::vector<hipcompStatus_t> q_statuses = host_copy(d_q_statuses, n);
    // the buffers and their twins
    std::vector<size_t> caps, rows;
    for (size_t i = 0; i < n; ++i) {
      caps.push_back(sized(c.items[i].cap, q_sizes[i], 77));
      rows.push_back(sized(c.items[i].rows, q_pages[i], 3));
    }
    Buffers all, one;
    all.plan(caps, rows, c.align);
    one.plan(caps, rows, c.align);
    auto pointers = [&](Buffers& b, std::vector<uint8_t*>& outs, std::vector<ParquetPageInfo*>& tabs) {
      for (size_t i = 0; i < n; ++i) {
        outs.push_back(b.outs.dev + b.outs.at[i]);
        tabs.push_back(reinterpret_cast<ParquetPageInfo*>(b.tables.dev + b.tables.at[i]));
      }
    };
    std::vector<uint8_t*> outs_all, outs_one;
    std::vector<ParquetPageInfo*> tabs_all, tabs_one;
    pointers(all, outs_all, tabs_all);
    pointers(one, outs_one, tabs_one);
    uint8_t** d_outs_all = device_copy(outs_all);
    uint8_t** d_outs_one = device_copy(outs_one);
    ParquetPageInfo** d_tabs_all = device_copy(tabs_all);
    ParquetPageInfo** d_tabs_one = device_copy(tabs_one);
    size_t* d_caps = device_copy(caps);
    size_t* d_rows = device_copy(rows);
    size_t* d_sizes = device_array<size_t>(2 * n);
    size_t* d_pages = device_array<size_t>(2 * n);
    hipcompStatus_t* d_statuses = device_array<hipcompStatus_t>(2 * n);
    HIP(hipMemset(d_sizes, 0xEE, 2 * n * sizeof(size_t)));
    HIP(hipMemset(d_pages, 0xEE, 2 * n * sizeof(size_t)));
    HIP(hipMemset(d_statuses, 0xEE, 2 * n * sizeof(hipcompStatus_t)));
    m.decompress_parquet_pages(d_chunk_ptrs, d_chunk_bytes, d_outs_all, d_caps, d_sizes, d_statuses, c.tables ? d_tabs_all : nullptr,
                               c.tables ? d_rows : nullptr, d_pages, n, codec);
    HIP(hipStreamSynchronize(stream));
    const hipcomp::ParquetPagesStats stats = m.get_parquet_pages_stats();
    if (c.ones)
      for (size_t i = 0; i < n; ++i)
        m.decompress_parquet_pages(d_chunk_ptrs + i, d_chunk_bytes + i, d_outs_one + i, d_caps + i, d_sizes + n + i,
                                   d_statuses + n + i, c.tables ? d_tabs_one + i : nullptr, c.tables ? d_rows + i : nullptr,
                                   d_pages + n + i, 1, codec);
    HIP(hipStreamSynchronize(stream));
    all.fetch();
    one.fetch();
    const std::vector<size_t> sizes = host_copy(d_sizes, 2 * n), pages = host_copy(d_pages, 2 * n);
    const std::vector<hipcompStatus_t> statuses = host_copy(d_statuses, 2 * n);
    std::ofstream out(c.outfile, std::ios::binary);
    for (size_t i = 0; i < n; ++i) {
      // (a size or a count that is out of its buffer is told as it is, and nothing of it written to the file)
      const bool fits = sizes[i] <= caps[i] && (!c.tables || pages[i] <= rows[i]);
      int eq_one = -1;
      if (c.ones)
        eq_one = statuses[i] == statuses[n + i] && sizes[i] == sizes[n + i] && pages[i] == pages[n + i] && fits
                 && std::memcmp(&all.h_outs[all.outs.at[i]], &one.h_outs[one.outs.at[i]], sizes[i]) == 0
                 && (!c.tables
                     || std::memcmp(&all.h_tables[all.tables.at[i]], &one.h_tables[one.tables.at[i]], pages[i] * kRow) == 0)
                 && one.guards(i);
      std::printf("item %zu status %d size %zu pages %zu q_status %d q_size %zu q_pages %zu guards %d untouched %d one_status %d "
                  "one_size %zu one_pages %zu eq_one %d\n",
                  i, (int)statuses[i], sizes[i], pages[i], (int)q_statuses[i], q_sizes[i], q_pages[i], all.guards(i) ? 1 : 0,
                  all.untouched(i) ? 1 : 0, c.ones ? (int)statuses[n + i] : -1, c.ones ? sizes[n + i] : 0, c.ones ? pages[n + i] : 0,
                  eq_one);
      if (fits) {
        out.write(reinterpret_cast<const char*>(&all.h_outs[all.outs.at[i]]), (std::streamsize)sizes[i]);
        if (c.tables)
          out.write(reinterpret_cast<const char*>(&all.h_tables[all.tables.at[i]]), (std::streamsize)(pages[i] * kRow));
      }
    }
    if (scratch) {
      const std::vector<uint8_t> behind = host_copy(scratch + scratch_bytes, kGuard);
      intact = all_fill(behind.data(), kGuard) ? 1 : 0;
    }
    std::printf("case %zu scratch_intact %d stats_pages %zu passes %zu pass_pages %zu\n", number, intact, stats.pages, stats.passes,
                stats.pass_pages);
    for (void* p : {(void*)d_chunk_ptrs, (void*)d_chunk_bytes, (void*)d_q_pages, (void*)d_q_sizes, (void*)d_q_statuses, (void*)d_outs_all,
                    (void*)d_outs_one, (void*)d_tabs_all, (void*)d_tabs_one, (void*)d_caps, (void*)d_rows, (void*)d_sizes, (void*)d_pages,
                    (void*)d_statuses})
      (void)hipFree(p);
    HIP(hipDeviceSynchronize());
    // (the manager goes before a caller's scratch does)
    if (scratch) {
      m.set_scratch_buffer(nullptr);
      (void)hipFree(scratch);
    }
  }
  HIP(hipStreamDestroy(stream));
  return 0;
}

int misuse()
{
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  int threw = 0, quiet = 0;
  {
    // a manager of small chunks has a small scratch: a caller's buffer of that size does not hold 2^20 chunks' states
    hipcomp::SnappyManager m(64, stream, 0);
    uint8_t* scratch = nullptr;
    HIP(hipMalloc((void**)&scratch, m.get_required_scratch_buffer_size()));
    m.set_scratch_buffer(scratch);
    const size_t room = m.get_required_scratch_buffer_size();
    const size_t n = room / 128 + 1; // (parquet_pages_plan.hpp: 128 bytes of state per chunk)
    void* any = scratch;             // (never read: the call throws before a launch)
    try {
      if (n <= (size_t(1) << 20))
        m.decompress_parquet_pages((const uint8_t* const*)any, (const size_t*)any, (uint8_t* const*)any, (const size_t*)any,
                                   (size_t*)any, (hipcompStatus_t*)any, nullptr, nullptr, (size_t*)any, n, ParquetCodec::Snappy);
    } catch (const std::runtime_error&) {
      threw |= 1;
    }
    try {
      m.decompress_parquet_pages(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                                 ParquetCodec::Snappy);
    } catch (const std::runtime_error&) {
      threw |= 2;
    }
    try {
      m.get_parquet_pages_sizes(nullptr, nullptr, nullptr, nullptr, nullptr, (size_t(1) << 20) + 1, ParquetCodec::Snappy);
    } catch (const std::runtime_error&) {
      threw |= 4;
    }
    // no chunks: nothing to do, nothing looked at
    m.decompress_parquet_pages(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, ParquetCodec::Snappy);
    m.get_parquet_pages_sizes(nullptr, nullptr, nullptr, nullptr, nullptr, 0, ParquetCodec::Uncompressed);
    quiet = 1;
    std::printf("threw %d quiet %d items %zu states_chunks %zu\n", threw, quiet, m.get_parquet_pages_stats().items, n);
    HIP(hipDeviceSynchronize());
    m.set_scratch_buffer(nullptr);
    (void)hipFree(scratch);
  }
  HIP(hipStreamDestroy(stream));
  return 0;
}

// ---- timing ---------------------------------------------------------------------------------------------------
// The host walk of today's way, kept apart from the library's: a Thrift reader of what the generator's writer writes
// for a V1 data page (i32 fields 1-4 and the struct 5 of four i32s), as a user's code would have it.
struct HostPage
{
  size_t body = 0, csize = 0, usize = 0;
};
bool host_walk(const std::vector<uint8_t>& d, std::vector<HostPage>& pages)
{
  size_t pos = 0;
  auto varint = [&](uint64_t& v) {
    v = 0;
    for (int shift = 0; pos < d.size() && shift < 64; shift += 7) {
      const uint8_t b = d[pos++];
      v |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80))
        return true;
    }
    return false;
  };
  while (pos < d.size()) {
    int depth = 0;
    uint32_t id[2] = {0, 0};
    int64_t top[5] = {0, 0, 0, 0, 0};
    for (;;) {
      if (pos >= d.size())
        return false;
      const uint8_t h = d[pos++];
      if (h == 0) {
        if (depth == 0)
          break;
        --depth;
        continue;
      }
      if ((h >> 4) == 0)
        return false; // (the generator's writer uses deltas here)
      id[depth] += h >> 4;
      const uint32_t type = h & 15;
      if (type == 5) {
        uint64_t u;
        if (!varint(u))
          return false;
        if (depth == 0 && id[0] <= 4)
          top[id[0]] = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
      } else if (type == 12 && depth == 0) {
        depth = 1;
        id[1] = 0;
      } else {
        return false;
      }
    }
    HostPage p;
    p.body = pos;
    p.usize = (size_t)top[2];
    p.csize = (size_t)top[3];
    if (p.csize > d.size() - pos)
      return false;
    pos += p.csize;
    pages.push_back(p);
  }
  return true;
}

int time_case(const char* list, int reps)
{
  const std::vector<Case> cases = read_cases(list);
  if (cases.size() != 1)
    return 2;
  const Case& c = cases[0];
  const size_t n = c.items.size();
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  {
    hipcomp::SnappyManager m(65536, stream, 0, (hipcomp::ChecksumPolicy)c.policy);
    Arena in;
    std::vector<size_t> lens;
    for (const ItemSpec& it : c.items)
      lens.push_back(it.data.size());
    in.plan(lens, kGuard, 0);
    std::vector<const uint8_t*> chunk_ptrs;
    for (size_t i = 0; i < n; ++i) {
      HIP(hipMemcpy(in.dev + in.at[i], c.items[i].data.data(), lens[i], hipMemcpyHostToDevice));
      chunk_ptrs.push_back(in.dev + in.at[i]);
    }
    const uint8_t** d_chunk_ptrs = device_copy(chunk_ptrs);
    size_t* d_chunk_bytes = device_copy(lens);
    // capacities from a host walk (both ways get the same buffers)
    std::vector<size_t> caps;
    size_t total_pages = 0, total_out = 0;
    for (size_t i = 0; i < n; ++i) {
      std::vector<HostPage> pages;
      if (!host_walk(c.items[i].data, pages))
        return 4;
      size_t sum = 0;
      for (const HostPage& p : pages)
        sum += p.usize;
      caps.push_back(sum);
      total_pages += pages.size();
      total_out += sum;
    }
    Buffers a, b;
    a.plan(caps, std::vector<size_t>(n, 0), 0);
    b.plan(caps, std::vector<size_t>(n, 0), 0);
    std::vector<uint8_t*> outs_a, outs_b;
    for (size_t i = 0; i < n; ++i) {
      outs_a.push_back(a.outs.dev + a.outs.at[i]);
      outs_b.push_back(b.outs.dev + b.outs.at[i]);
    }
    uint8_t** d_outs_a = device_copy(outs_a);
    size_t* d_caps = device_copy(caps);
    size_t* d_sizes = device_array<size_t>(n);
    size_t* d_pages = device_array<size_t>(n);
    hipcompStatus_t* d_statuses = device_array<hipcompStatus_t>(n);
    // today's way: its device arrays are allocated once, filled per call from the host walk
    const uint8_t** d_comp_ptrs = device_array<const uint8_t*>(total_pages);
    size_t* d_comp_bytes = device_array<size_t>(total_pages);
    size_t* d_out_bytes = device_array<size_t>(total_pages);
    size_t* d_actual = device_array<size_t>(total_pages);
    uint8_t** d_out_ptrs = device_array<uint8_t*>(total_pages);
    hipcompStatus_t* d_page_statuses = device_array<hipcompStatus_t>(total_pages);
    size_t temp_bytes = 0;
    hipcompBatchedSnappyDecompressGetTempSize(total_pages, 65536, &temp_bytes);
    void* d_temp = device_array<uint8_t>(temp_bytes);
    hipEvent_t e0, e1;
    HIP(hipEventCreate(&e0));
    HIP(hipEventCreate(&e1));
    std::vector<float> ms_one, ms_today;
    for (int r = 0; r < reps + 1; ++r) {
      float ms = 0;
      HIP(hipEventRecord(e0, stream));
      m.decompress_parquet_pages(d_chunk_ptrs, d_chunk_bytes, d_outs_a, d_caps, d_sizes, d_statuses, nullptr, nullptr, d_pages, n,
                                 ParquetCodec::Snappy);
      HIP(hipEventRecord(e1, stream));
      HIP(hipEventSynchronize(e1));
      HIP(hipEventElapsedTime(&ms, e0, e1));
      if (r)
        ms_one.push_back(ms);
      HIP(hipEventRecord(e0, stream));
      {
        std::vector<const uint8_t*> comp_ptrs;
        std::vector<size_t> comp_bytes, out_bytes;
        std::vector<uint8_t*> out_ptrs;
        for (size_t i = 0; i < n; ++i) {
          std::vector<HostPage> pages;
          (void)host_walk(c.items[i].data, pages);
          size_t at = 0;
          for (const HostPage& p : pages) {
            comp_ptrs.push_back(chunk_ptrs[i] + p.body);
            comp_bytes.push_back(p.csize);
            out_bytes.push_back(p.usize);
            out_ptrs.push_back(outs_b[i] + at);
            at += p.usize;
          }
        }
        HIP(hipMemcpyAsync(d_comp_ptrs, comp_ptrs.data(), total_pages * 8, hipMemcpyHostToDevice, stream));
        HIP(hipMemcpyAsync(d_comp_bytes, comp_bytes.data(), total_pages * 8, hipMemcpyHostToDevice, stream));
        HIP(hipMemcpyAsync(d_out_bytes, out_bytes.data(), total_pages * 8, hipMemcpyHostToDevice, stream));
        HIP(hipMemcpyAsync(d_out_ptrs, out_ptrs.data(), total_pages * 8, hipMemcpyHostToDevice, stream));
        if (hipcompBatchedSnappyDecompressAsync((const void* const*)d_comp_ptrs, d_comp_bytes, d_out_bytes, d_actual, total_pages, d_temp,
                                                temp_bytes, (void* const*)d_out_ptrs, d_page_statuses, stream)
            != hipcompSuccess)
          return 4;
        HIP(hipStreamSynchronize(stream)); // (the host vectors go out of scope)
      }
      HIP(hipEventRecord(e1, stream));
      HIP(hipEventSynchronize(e1));
      HIP(hipEventElapsedTime(&ms, e0, e1));
      if (r)
        ms_today.push_back(ms);
    }
    a.fetch();
    b.fetch();
    const std::vector<hipcompStatus_t> statuses = host_copy(d_statuses, n);
    size_t same = 0;
    for (size_t i = 0; i < n; ++i)
      same += statuses[i] == hipcompSuccess && std::memcmp(&a.h_outs[a.outs.at[i]], &b.h_outs[b.outs.at[i]], caps[i]) == 0 ? 1 : 0;
    std::sort(ms_one.begin(), ms_one.end());
    std::sort(ms_today.begin(), ms_today.end());
    std::printf("chunks %zu pages %zu out_bytes %zu same %zu one_call_ms %.4f today_ms %.4f passes %zu\n", n, total_pages, total_out,
                same, ms_one[ms_one.size() / 2], ms_today[ms_today.size() / 2], m.get_parquet_pages_stats().passes);
    HIP(hipDeviceSynchronize());
  }
  HIP(hipStreamDestroy(stream));
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  try {
    if (argc == 3 && std::string(argv[1]) == "batch") {
      const std::vector<Case> cases = read_cases(argv[2]);
      for (size_t k = 0; k < cases.size(); ++k)
        if (const int r = run_case(k, cases[k]))
          return r;
      return 0;
    }
    if (argc == 2 && std::string(argv[1]) == "misuse")
      return misuse();
    if (argc == 4 && std::string(argv[1]) == "time")
      return time_case(argv[2], std::atoi(argv[3]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 6;
  }
  return 2;
}
