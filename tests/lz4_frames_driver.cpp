// Batches of LZ4 frames in one call (hipcomp/lz4.hpp: decompress_frames, get_frames_decompressed_sizes) driven on
// files, for tests/test_lz4_frames_gpu.py and scripts/quick_lz4_frames.py.  Written against include/ and linked to
// libhipcomp.so.
//   lz4_frames_driver batch LIST
//       LIST holds cases.  A case is a line "case POLICY PREFIX scratch|own PASS_ENTRIES SANDWICH OUT N" and N lines
//       "FILE OFFSET LENGTH CAPACITY": item i is bytes [OFFSET, OFFSET + LENGTH) of FILE (LENGTH -1: to its end); every
//       FILE is copied to the device once, 3 bytes behind a 256-byte boundary, and the items stand where they stand in
//       it.  CAPACITY: a number, or E (exact: what the size query says for the item on its own), S (one short of it),
//       O (77 more).  PREFIX 0: none, 1: the Arrow length.  PASS_ENTRIES: set_frames_pass_entries.
//       Every item gets an output buffer of exactly its capacity between guard bytes, at an odd address.  Per item,
//       in this order and all under one manager: (PREFIX 0 only) configure_frame_decompression + decompress_frame of
//       the item's bytes into a buffer of exactly decomp_data_size bytes; decompress_frames of the item alone; then
//       the size query and decompress_frames of the whole batch.  SANDWICH 1: the decompress_frame of every item is
//       run once more behind the batch and has to give what it gave in front of it.  OUT gets the batch's outputs, item
//       after item, each `size` bytes.
//       prints per item "item I single_status A single_size B one_status C one_size D status E size F query G
//       eq_single H eq_one J guards K" (H, J: the batch's bytes of the item equal the single read's / the one-item
//       batch's; -1 where there is nothing to compare: another size, or no single read) and per case
//       "case 1 items N blocks B passes P pass_entries Q scratch_guard H sandwich S" (S: -1 not asked, 1 same, 0 not).
//   lz4_frames_driver limit CHUNK N
//       a manager of CHUNK-byte chunks with a caller-owned scratch; decompress_frames of N empty Arrow items.
//       prints "scratch_bytes S threw T worst_status W scratch_guard H untouched U stats_items I" (U: the first MiB of
//       the scratch and the two result arrays, filled with 0xEE before the call, are as they were behind it)
//   lz4_frames_driver nothing
//       num_items == 0 with null arrays; prints "threw T items N"
//   lz4_frames_driver unchanged FILE
//       a manager writes FILE's bytes as an indexed frame; decompress_frame and decompress_frame_range of it before
//       and behind a decompress_frames of [that frame, that frame]; prints "frame_same A range_same B batch_worst W"
//   lz4_frames_driver timing ITEMS LINKED REPS FILE
//       see scripts/quick_lz4_frames.py
#include "hipcomp/lz4.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define HIP(x)                                                                                                         \
  do {                                                                                                                 \
    hipError_t e_ = (x);                                                                                               \
    if (e_ != hipSuccess) {                                                                                            \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                                                     \
      std::exit(3);                                                                                                    \
    }                                                                                                                  \
  } while (0)

using hipcomp::LZ4FramePrefix;

static std::vector<uint8_t> read_file(const std::string& path)
{
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f)
    std::exit(2);
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> v((size_t)n);
  if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n)
    std::exit(2);
  std::fclose(f);
  return v;
}

constexpr size_t kGuard = 64, kScratchGuard = 256;
constexpr uint8_t kGuardByte = 0xA5, kScratchGuardByte = 0x5C;

// `bytes` bytes 1 byte behind a 256-byte boundary, kGuard guard bytes in front and behind
struct Guarded
{
  uint8_t* base = nullptr;
  uint8_t* at = nullptr;
  size_t bytes = 0, total = 0;
  explicit Guarded(size_t n) : bytes(n), total(kGuard + 1 + n + kGuard)
  {
    HIP(hipMalloc((void**)&base, total));
    HIP(hipMemset(base, kGuardByte, total));
    at = base + kGuard + 1;
  }
  Guarded(const Guarded&) = delete;
  ~Guarded() { (void)hipFree(base); }
  // the first `n` bytes of [at, at + bytes) into h; true: everything around the buffer is as it was
  bool fetch(std::vector<uint8_t>& h, size_t n) const
  {
    std::vector<uint8_t> all(total);
    HIP(hipMemcpy(all.data(), base, total, hipMemcpyDeviceToHost));
    const size_t a = (size_t)(at - base);
    bool intact = true;
    for (size_t i = 0; i < total; ++i)
      if ((i < a || i >= a + bytes) && all[i] != kGuardByte)
        intact = false;
    h.assign(all.begin() + a, all.begin() + a + std::min(n, bytes));
    return intact;
  }
};

struct Scratch
{
  uint8_t* p = nullptr;
  size_t bytes = 0;
  void give(hipcomp::LZ4Manager& m)
  {
    bytes = m.get_required_scratch_buffer_size();
    HIP(hipMalloc((void**)&p, bytes + kScratchGuard));
    HIP(hipMemset(p + bytes, kScratchGuardByte, kScratchGuard));
    m.set_scratch_buffer(p);
  }
  bool intact() const
  {
    if (!p)
      return true;
    std::vector<uint8_t> g(kScratchGuard);
    HIP(hipMemcpy(g.data(), p + bytes, kScratchGuard, hipMemcpyDeviceToHost));
    return std::all_of(g.begin(), g.end(), [](uint8_t b) { return b == kScratchGuardByte; });
  }
  ~Scratch() { (void)hipFree(p); }
};

// the six arrays of a call on the device
struct Arrays
{
  size_t n;
  uint8_t* d = nullptr;
  const uint8_t** item_ptrs;
  size_t* item_bytes;
  uint8_t** out_ptrs;
  size_t* caps;
  size_t* actual;
  hipcompStatus_t* statuses;
  Arrays(const std::vector<const uint8_t*>& ip, const std::vector<size_t>& ib, const std::vector<uint8_t*>& op,
         const std::vector<size_t>& oc)
      : n(ip.size())
  {
    const size_t m = n ? n : 1;
    HIP(hipMalloc((void**)&d, m * 44));
    HIP(hipMemset(d, 0xEE, m * 44));
    item_ptrs = (const uint8_t**)d;
    item_bytes = (size_t*)(d + 8 * m);
    out_ptrs = (uint8_t**)(d + 16 * m);
    caps = (size_t*)(d + 24 * m);
    actual = (size_t*)(d + 32 * m);
    statuses = (hipcompStatus_t*)(d + 40 * m);
    if (n) {
      HIP(hipMemcpy(item_ptrs, ip.data(), 8 * n, hipMemcpyHostToDevice));
      HIP(hipMemcpy(item_bytes, ib.data(), 8 * n, hipMemcpyHostToDevice));
      HIP(hipMemcpy(out_ptrs, op.data(), 8 * n, hipMemcpyHostToDevice));
      HIP(hipMemcpy(caps, oc.data(), 8 * n, hipMemcpyHostToDevice));
    }
  }
  Arrays(const Arrays&) = delete;
  ~Arrays() { (void)hipFree(d); }
  std::vector<size_t> sizes() const
  {
    std::vector<size_t> v(n);
    if (n)
      HIP(hipMemcpy(v.data(), actual, 8 * n, hipMemcpyDeviceToHost));
    return v;
  }
  std::vector<int> status() const
  {
    std::vector<hipcompStatus_t> v(n);
    if (n)
      HIP(hipMemcpy(v.data(), statuses, sizeof(hipcompStatus_t) * n, hipMemcpyDeviceToHost));
    return std::vector<int>(v.begin(), v.end());
  }
};

struct DeviceFile
{
  uint8_t* base = nullptr;
  uint8_t* at = nullptr;
  size_t bytes = 0;
};

struct Single
{
  int status = -1;
  size_t size = 0;
  std::vector<uint8_t> bytes;
  bool guards = true;
};

static Single single_read(hipcomp::LZ4Manager& m, const uint8_t* d_in, size_t n)
{
  Single s;
  hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(d_in, n);
  Guarded out(cfg.decomp_data_size);
  m.decompress_frame(out.at, d_in, n, cfg);
  HIP(hipDeviceSynchronize());
  s.status = (int)*cfg.get_status();
  s.size = cfg.decomp_data_size;
  s.guards = out.fetch(s.bytes, s.size);
  return s;
}

static int batch_cases(const char* list_path)
{
  std::ifstream list(list_path);
  std::map<std::string, DeviceFile> files;
  std::string text;
  while (std::getline(list, text)) {
    if (text.empty())
      continue;
    std::istringstream head(text);
    std::string word, scratch_word, out_path;
    int policy = 0, prefix_word = 0, sandwich = 0;
    size_t pass_entries = 0, n = 0;
    head >> word >> policy >> prefix_word >> scratch_word >> pass_entries >> sandwich >> out_path >> n;
    if (word != "case")
      std::exit(2);
    const LZ4FramePrefix prefix = prefix_word ? LZ4FramePrefix::ArrowLength : LZ4FramePrefix::None;
    hipcomp::LZ4Manager m(65536, HIPCOMP_TYPE_CHAR, 0, 0, (hipcomp::ChecksumPolicy)policy);
    Scratch scratch;
    if (scratch_word == "scratch")
      scratch.give(m);
    m.set_frames_pass_entries(pass_entries);
    std::vector<const uint8_t*> ip(n);
    std::vector<size_t> ib(n), oc(n);
    std::vector<std::string> cap_words(n);
    for (size_t i = 0; i < n; ++i) {
      std::getline(list, text);
      std::istringstream line(text);
      std::string path;
      long long offset = 0, length = 0;
      line >> path >> offset >> length >> cap_words[i];
      DeviceFile& f = files[path];
      if (!f.base) {
        const std::vector<uint8_t> data = read_file(path);
        f.bytes = data.size();
        HIP(hipMalloc((void**)&f.base, f.bytes + 512));
        HIP(hipMemset(f.base, 0x04, f.bytes + 512));
        f.at = f.base + 256 + 3;
        if (f.bytes)
          HIP(hipMemcpy(f.at, data.data(), f.bytes, hipMemcpyHostToDevice));
      }
      ip[i] = f.at + offset;
      ib[i] = length < 0 ? f.bytes - (size_t)offset : (size_t)length;
    }
    // the items on their own: the single read, the size query, the one-item batch
    std::vector<Single> singles(n), ones(n);
    std::vector<int> one_status(n);
    for (size_t i = 0; i < n; ++i) {
      if (prefix == LZ4FramePrefix::None)
        singles[i] = single_read(m, ip[i], ib[i]);
      const std::vector<const uint8_t*> p1{ip[i]};
      const std::vector<size_t> b1{ib[i]};
      size_t exact = 0;
      {
        Arrays q(p1, b1, {nullptr}, {0});
        m.get_frames_decompressed_sizes(q.item_ptrs, q.item_bytes, q.actual, 1, prefix);
        HIP(hipDeviceSynchronize());
        exact = q.sizes()[0];
      }
      const std::string& c = cap_words[i];
      oc[i] = c == "E" ? exact : c == "S" ? (exact ? exact - 1 : 0) : c == "O" ? exact + 77 : std::strtoull(c.c_str(), nullptr, 0);
      Guarded out(oc[i]);
      Arrays a(p1, b1, {out.at}, {oc[i]});
      m.decompress_frames(a.item_ptrs, a.item_bytes, a.out_ptrs, a.caps, a.actual, a.statuses, 1, prefix);
      HIP(hipDeviceSynchronize());
      ones[i].status = a.status()[0];
      ones[i].size = a.sizes()[0];
      ones[i].guards = out.fetch(ones[i].bytes, ones[i].size);
    }
    // the batch
    std::vector<std::unique_ptr<Guarded>> outs;
    std::vector<uint8_t*> op(n);
    for (size_t i = 0; i < n; ++i) {
      outs.emplace_back(new Guarded(oc[i]));
      op[i] = outs[i]->at;
    }
    Arrays a(ip, ib, op, oc);
    Arrays q(ip, ib, op, oc);
    m.get_frames_decompressed_sizes(q.item_ptrs, q.item_bytes, q.actual, n, prefix);
    m.decompress_frames(a.item_ptrs, a.item_bytes, a.out_ptrs, a.caps, a.actual, a.statuses, n, prefix);
    HIP(hipDeviceSynchronize());
    const hipcomp::LZ4FramesStats stats = m.get_frames_stats();
    const std::vector<size_t> sizes = a.sizes(), query = q.sizes();
    const std::vector<int> status = a.status();
    FILE* out_file = std::fopen(out_path.c_str(), "wb");
    if (!out_file)
      std::exit(2);
    for (size_t i = 0; i < n; ++i) {
      std::vector<uint8_t> got;
      const bool guards = outs[i]->fetch(got, sizes[i]) && ones[i].guards && singles[i].guards;
      if (!got.empty() && std::fwrite(got.data(), 1, got.size(), out_file) != got.size())
        std::exit(2);
      const int eq_single = prefix != LZ4FramePrefix::None || singles[i].size != sizes[i] ? -1 : got == singles[i].bytes ? 1 : 0;
      const int eq_one = ones[i].size != sizes[i] ? -1 : got == ones[i].bytes ? 1 : 0;
      std::printf("item %zu single_status %d single_size %zu one_status %d one_size %zu status %d size %zu query %zu eq_single %d "
                  "eq_one %d guards %d\n",
                  i, singles[i].status, singles[i].size, ones[i].status, ones[i].size, status[i], sizes[i], query[i], eq_single,
                  eq_one, guards ? 1 : 0);
    }
    std::fclose(out_file);
    int same = -1;
    if (sandwich && prefix == LZ4FramePrefix::None) {
      same = 1;
      for (size_t i = 0; i < n; ++i) {
        const Single again = single_read(m, ip[i], ib[i]);
        if (again.status != singles[i].status || again.size != singles[i].size || again.bytes != singles[i].bytes || !again.guards)
          same = 0;
      }
    }
    std::printf("case 1 items %zu blocks %zu passes %zu pass_entries %zu scratch_guard %d sandwich %d\n", stats.items, stats.blocks,
                stats.passes, stats.pass_entries, scratch.intact() ? 1 : 0, same);
    std::fflush(stdout);
  }
  for (auto& f : files)
    (void)hipFree(f.second.base);
  return 0;
}

static int limit(size_t chunk, size_t n)
{
  hipcomp::LZ4Manager m(chunk, HIPCOMP_TYPE_CHAR, 0, 0);
  Scratch scratch;
  scratch.give(m);
  uint8_t* d_dummy = nullptr;
  HIP(hipMalloc((void**)&d_dummy, 64));
  const std::vector<const uint8_t*> ip(n, d_dummy);
  const std::vector<size_t> ib(n, 0), oc(n, 0);
  const std::vector<uint8_t*> op(n, d_dummy);
  Arrays a(ip, ib, op, oc);
  // (the head of the scratch, where the items' state would go, and the result arrays are filled with 0xEE: a call
  // that throws before it launches anything leaves every byte of them as it is)
  const size_t head = std::min<size_t>(scratch.bytes, 1 << 20);
  HIP(hipMemset(scratch.p, 0xEE, head));
  int threw = 0, worst = 0, untouched = 1;
  try {
    m.decompress_frames(a.item_ptrs, a.item_bytes, a.out_ptrs, a.caps, a.actual, a.statuses, n, LZ4FramePrefix::ArrowLength);
    HIP(hipDeviceSynchronize());
    for (int s : a.status())
      worst = std::max(worst, s);
    for (size_t s : a.sizes())
      worst = std::max(worst, s ? 99 : 0);
  } catch (const std::runtime_error&) {
    threw = 1;
  }
  HIP(hipDeviceSynchronize());
  {
    std::vector<uint8_t> h(head), r(12 * n);
    HIP(hipMemcpy(h.data(), scratch.p, head, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(r.data(), (const uint8_t*)a.actual, 12 * n, hipMemcpyDeviceToHost)); // (actual and statuses lie back to back)
    for (uint8_t b : h)
      untouched &= b == 0xEE;
    for (uint8_t b : r)
      untouched &= b == 0xEE;
  }
  std::printf("scratch_bytes %zu threw %d worst_status %d scratch_guard %d untouched %d stats_items %zu\n", scratch.bytes, threw,
              worst, scratch.intact() ? 1 : 0, untouched, m.get_frames_stats().items);
  HIP(hipFree(d_dummy));
  return 0;
}

static int nothing()
{
  hipcomp::LZ4Manager m(65536, HIPCOMP_TYPE_CHAR, 0, 0);
  int threw = 0;
  try {
    m.decompress_frames(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, LZ4FramePrefix::None);
    m.get_frames_decompressed_sizes(nullptr, nullptr, nullptr, 0, LZ4FramePrefix::ArrowLength);
  } catch (const std::runtime_error&) {
    threw = 1;
  }
  int misuse = 0;
  try {
    m.decompress_frames(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, LZ4FramePrefix::None);
  } catch (const std::runtime_error&) {
    misuse += 1;
  }
  try {
    m.get_frames_decompressed_sizes(nullptr, nullptr, nullptr, (size_t(1) << 20) + 1, LZ4FramePrefix::None);
  } catch (const std::runtime_error&) {
    misuse += 1;
  }
  HIP(hipDeviceSynchronize());
  std::printf("threw %d items %zu misuse_threw %d\n", threw, m.get_frames_stats().items, misuse);
  return 0;
}

static int unchanged(const char* path)
{
  const std::vector<uint8_t> data = read_file(path);
  const size_t n = data.size();
  hipcomp::LZ4Manager m(65536, HIPCOMP_TYPE_CHAR, 0, 0, hipcomp::ComputeAndVerify);
  uint8_t *d_in = nullptr, *d_frame = nullptr;
  size_t* d_bytes = nullptr;
  HIP(hipMalloc((void**)&d_in, n + 16));
  HIP(hipMalloc((void**)&d_bytes, 8));
  HIP(hipMemcpy(d_in, data.data(), n, hipMemcpyHostToDevice));
  hipcomp::CompressionConfig ccfg = m.configure_frame_compression(n, hipcomp::LZ4FrameIndex::Leading);
  HIP(hipMalloc((void**)&d_frame, ccfg.max_compressed_buffer_size + 16));
  m.compress_frame(d_in, d_frame, ccfg, d_bytes, hipcomp::LZ4FrameIndex::Leading);
  HIP(hipDeviceSynchronize());
  size_t frame_bytes = 0;
  HIP(hipMemcpy(&frame_bytes, d_bytes, 8, hipMemcpyDeviceToHost));
  const size_t first = 100, count = n > 70100 ? 70000 : n / 2;
  struct Result
  {
    Single frame;
    int range_status;
    std::vector<uint8_t> range;
    bool range_guards;
  };
  const auto both = [&] {
    Result r;
    r.frame = single_read(m, d_frame, frame_bytes);
    hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(d_frame, frame_bytes);
    Guarded out(count);
    m.decompress_frame_range(out.at, d_frame, frame_bytes, cfg, first, count);
    HIP(hipDeviceSynchronize());
    r.range_status = (int)*cfg.get_status();
    r.range_guards = out.fetch(r.range, count);
    return r;
  };
  const Result before = both();
  int worst = 0;
  {
    Guarded o0(n), o1(n);
    Arrays a({d_frame, d_frame}, {frame_bytes, frame_bytes}, {o0.at, o1.at}, {n, n});
    m.decompress_frames(a.item_ptrs, a.item_bytes, a.out_ptrs, a.caps, a.actual, a.statuses, 2, LZ4FramePrefix::None);
    HIP(hipDeviceSynchronize());
    std::vector<uint8_t> h0, h1;
    const bool g = o0.fetch(h0, n) && o1.fetch(h1, n);
    for (int s : a.status())
      worst = std::max(worst, s);
    if (!g || h0 != data || h1 != data || a.sizes()[0] != n || a.sizes()[1] != n)
      worst = 99;
  }
  const Result after = both();
  const bool frame_same = before.frame.status == 0 && after.frame.status == 0 && before.frame.bytes == data
                          && after.frame.bytes == data && before.frame.guards && after.frame.guards;
  const std::vector<uint8_t> want(data.begin() + first, data.begin() + first + count);
  const bool range_same = before.range_status == 0 && after.range_status == 0 && before.range == want && after.range == want
                          && before.range_guards && after.range_guards;
  std::printf("frame_same %d range_same %d batch_worst %d\n", frame_same ? 1 : 0, range_same ? 1 : 0, worst);
  HIP(hipFree(d_in));
  HIP(hipFree(d_frame));
  HIP(hipFree(d_bytes));
  return 0;
}

// ---- timing (scripts/quick_lz4_frames.py) --------------------------------------------------------------------
// ITEMS copies of the frame in FILE (each at an address of its own) read by one decompress_frames call and by the
// loop of configure_frame_decompression + decompress_frame over the same items; 2 warm-up repetitions, the two ways
// alternate inside every repetition; HIP events around each.
static int timing(size_t items, const char* label, int reps, const char* path)
{
  const std::vector<uint8_t> frame = read_file(path);
  const size_t stride = (frame.size() + 8 + 255) & ~size_t(255);
  uint8_t* d_items = nullptr;
  HIP(hipMalloc((void**)&d_items, stride * items));
  for (size_t i = 0; i < items; ++i)
    HIP(hipMemcpy(d_items + i * stride, frame.data(), frame.size(), hipMemcpyHostToDevice));
  hipcomp::LZ4Manager m(65536, HIPCOMP_TYPE_CHAR, 0, 0);
  hipcomp::DecompressionConfig first = m.configure_frame_decompression(d_items, frame.size());
  const size_t size = first.decomp_data_size, out_stride = (size + 255) & ~size_t(255);
  uint8_t* d_out = nullptr;
  HIP(hipMalloc((void**)&d_out, out_stride * items + 16));
  std::vector<const uint8_t*> ip(items);
  std::vector<uint8_t*> op(items);
  for (size_t i = 0; i < items; ++i) {
    ip[i] = d_items + i * stride;
    op[i] = d_out + i * out_stride;
  }
  Arrays a(ip, std::vector<size_t>(items, frame.size()), op, std::vector<size_t>(items, size));
  hipEvent_t e0, e1;
  HIP(hipEventCreate(&e0));
  HIP(hipEventCreate(&e1));
  std::vector<float> ms[2];
  int worst = 0;
  for (int r = 0; r < reps + 2; ++r)
    for (int k = 0; k < 2; ++k) {
      float t = 0;
      HIP(hipEventRecord(e0, 0));
      if (k == 0) {
        m.decompress_frames(a.item_ptrs, a.item_bytes, a.out_ptrs, a.caps, a.actual, a.statuses, items, LZ4FramePrefix::None);
      } else {
        for (size_t i = 0; i < items; ++i) {
          hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(ip[i], frame.size());
          m.decompress_frame(op[i], ip[i], frame.size(), cfg);
          if (i + 1 == items) { // (the status is the device's word: read behind the events)
            HIP(hipEventRecord(e1, 0));
            HIP(hipEventSynchronize(e1));
            worst = std::max(worst, (int)*cfg.get_status());
          }
        }
      }
      if (k == 0) {
        HIP(hipEventRecord(e1, 0));
        HIP(hipEventSynchronize(e1));
        for (int s : a.status())
          worst = std::max(worst, s);
      }
      HIP(hipEventElapsedTime(&t, e0, e1));
      if (r >= 2)
        ms[k].push_back(t);
    }
  for (auto& v : ms)
    std::sort(v.begin(), v.end());
  const float batch = ms[0][ms[0].size() / 2], loop = ms[1][ms[1].size() / 2];
  std::printf("%s items %zu bytes_each %zu frame_bytes %zu batch_median_ms %.4f loop_median_ms %.4f ratio %.2f batch_min_ms %.4f "
              "loop_min_ms %.4f passes %zu worst_status %d\n",
              label, items, size, frame.size(), batch, loop, loop / batch, ms[0][0], ms[1][0], m.get_frames_stats().passes, worst);
  HIP(hipFree(d_items));
  HIP(hipFree(d_out));
  return 0;
}

int main(int argc, char** argv)
{
  try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "batch" && argc == 3)
      return batch_cases(argv[2]);
    if (cmd == "limit" && argc == 4)
      return limit(std::strtoull(argv[2], nullptr, 0), std::strtoull(argv[3], nullptr, 0));
    if (cmd == "nothing" && argc == 2)
      return nothing();
    if (cmd == "unchanged" && argc == 3)
      return unchanged(argv[2]);
    if (cmd == "timing" && argc == 6)
      return timing(std::strtoull(argv[2], nullptr, 0), argv[3], std::atoi(argv[4]), argv[5]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 4;
  }
  std::fprintf(stderr, "usage: see the head of lz4_frames_driver.cpp\n");
  return 2;
}
