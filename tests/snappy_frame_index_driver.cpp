// The Snappy manager's seekable framed streams (hipcomp/snappy.hpp: compress_frame with SnappyFrameIndex::Leading,
// the indexed read inside configure_frame_decompression / decompress_frame, decompress_frame_range) driven on files,
// for tests/test_snappy_frame_index_gpu.py and scripts/quick_snappy_frame_index.py.  Written against include/ and
// linked to libhipcomp.so.
//   snappy_frame_index_driver write LIST
//       every line of LIST: CHUNK POLICY IN FRAME PLAIN scratch|own OFF
//       A manager of CHUNK-byte chunks with the ChecksumPolicy POLICY compresses the file IN (placed OFF bytes behind
//       a 256-byte boundary) in this process: with the call that has always been there to PLAIN, with
//       SnappyFrameIndex::None (compared with PLAIN) and with Leading, OFF bytes behind a 256-byte boundary between
//       guard bytes into a buffer of exactly max_compressed_buffer_size bytes, to FRAME.  Then FRAME is read back by
//       decompress_frame.
//       prints "status S frame_bytes F bound B plain_bytes P plain_bound Q guards G scratch_guard H roundtrip R walked W"
//       (R: 1 = decompress_frame gave status 0 and the input back; W: chunks its walk listed)
//   snappy_frame_index_driver read LIST
//       every line of LIST: CHUNK POLICY IN OUT scratch|own OFF_IN OFF_OUT
//       configure_frame_decompression + decompress_frame of the file IN (OFF_IN bytes behind a 256-byte boundary,
//       in an allocation that ends with it) by a manager of CHUNK-byte chunks into a buffer of exactly
//       decomp_data_size bytes OFF_OUT bytes behind a 256-byte boundary between guard bytes; OUT gets those bytes.
//       prints "configured C status S size D chunks N guards G scratch_guard H walked W"
//   snappy_frame_index_driver read_displaced LIST
//       `read`, but between configure_frame_decompression of IN and decompress_frame the manager configures another
//       buffer: decompress_frame then has no word of the host's on whether IN is indexed (a caller that configures
//       once and reads several buffers, or keeps a configuration) and decides everything on the device.
//   snappy_frame_index_driver range LIST
//       every line of LIST: CHUNK POLICY IN OUT scratch|own OFF_IN OFF_OUT FIRST COUNT
//       configure_frame_decompression + decompress_frame_range of bytes [FIRST, FIRST + COUNT) of the file IN into a
//       buffer of exactly COUNT bytes OFF_OUT bytes behind a 256-byte boundary between guard bytes, itself filled
//       with the guard byte; OUT gets those bytes.
//       prints "configured C status S size D guards G scratch_guard H untouched U walked W" (U: out holds nothing
//       but the guard byte)
//   snappy_frame_index_driver limits
//       prints "chunks N status S bound B chunks_configured C" for a manager of one-byte chunks and inputs of
//       4 194 294 and 4 194 295 bytes under Leading, and of the latter under None (nothing is compressed)
//   snappy_frame_index_driver timing DATA|- CHUNKS REPS
//       see scripts/quick_snappy_frame_index.py
//   snappy_frame_index_driver timing_plain DATA|- CHUNKS REPS configured|displaced
//       the stream without an index alone, the calls and their order those of snappy_frame_driver's `timing` (what a
//       call finds in the caches depends on the calls before it): for a comparison with another build of the library.
//       displaced: another buffer is configured behind the stream, so every read launches the indexed passes first.
#include "hipcomp/snappy.h"
#include "hipcomp/snappy.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

using Index = hipcomp::SnappyFrameIndex;

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

static void write_file(const std::string& path, const uint8_t* p, size_t n)
{
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || (n && std::fwrite(p, 1, n, f) != n))
    std::exit(2);
  std::fclose(f);
}

constexpr size_t kGuard = 256, kScratchGuard = 256;
constexpr uint8_t kGuardByte = 0xA5, kScratchGuardByte = 0x5C;

// `bytes` bytes `off` bytes behind a 256-byte boundary, kGuard guard bytes in front and behind
struct Guarded
{
  uint8_t* base = nullptr;
  uint8_t* at = nullptr;
  size_t bytes = 0, total = 0;
  Guarded(size_t n, size_t off) : bytes(n), total(256 + kGuard + n + kGuard + 16)
  {
    HIP(hipMalloc((void**)&base, total));
    HIP(hipMemset(base, kGuardByte, total));
    at = base + 256 + off;
  }
  ~Guarded() { (void)hipFree(base); }
  // the bytes of [at, at + bytes) into h; true: everything around them is as it was
  bool fetch(std::vector<uint8_t>& h) const
  {
    std::vector<uint8_t> all(total);
    HIP(hipMemcpy(all.data(), base, total, hipMemcpyDeviceToHost));
    const size_t a = (size_t)(at - base);
    bool intact = true;
    for (size_t i = 0; i < total; ++i)
      if ((i < a || i >= a + bytes) && all[i] != kGuardByte)
        intact = false;
    h.assign(all.begin() + a, all.begin() + a + bytes);
    return intact;
  }
};

struct Scratch
{
  uint8_t* p = nullptr;
  size_t bytes = 0;
  void give(hipcomp::SnappyManager& m)
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

static size_t fetch_size(const size_t* d)
{
  size_t v = 0;
  HIP(hipMemcpy(&v, d, 8, hipMemcpyDeviceToHost));
  return v;
}

static void write_one(std::istringstream& line)
{
  size_t chunk = 0, off = 0;
  int policy = 0;
  std::string in_path, frame_path, plain_path, scratch_word;
  line >> chunk >> policy >> in_path >> frame_path >> plain_path >> scratch_word >> off;
  const std::vector<uint8_t> data = read_file(in_path);
  hipcomp::SnappyManager m(chunk, 0, 0, (hipcomp::ChecksumPolicy)policy);
  Scratch scratch;
  if (scratch_word == "scratch")
    scratch.give(m);
  uint8_t* d_in_base = nullptr;
  HIP(hipMalloc((void**)&d_in_base, data.size() + 512));
  uint8_t* const d_in = d_in_base + off;
  if (!data.empty())
    HIP(hipMemcpy(d_in, data.data(), data.size(), hipMemcpyHostToDevice));
  size_t* d_bytes = nullptr;
  HIP(hipMalloc((void**)&d_bytes, 8));
  HIP(hipMemset(d_bytes, 0xEE, 8));
  // the stream without an index, by the call that has always been there
  hipcomp::CompressionConfig plain_cfg = m.configure_frame_compression(data.size());
  Guarded plain(plain_cfg.max_compressed_buffer_size, off);
  m.compress_frame(d_in, plain.at, plain_cfg, d_bytes);
  HIP(hipDeviceSynchronize());
  size_t plain_bytes = fetch_size(d_bytes);
  std::vector<uint8_t> h;
  bool guards = plain.fetch(h);
  if (plain_bytes <= h.size())
    write_file(plain_path, h.data(), plain_bytes);
  // ... and by the new call with None: the same bytes
  {
    hipcomp::CompressionConfig c = m.configure_frame_compression(data.size(), Index::None);
    Guarded again(c.max_compressed_buffer_size, off);
    m.compress_frame(d_in, again.at, c, d_bytes, Index::None);
    HIP(hipDeviceSynchronize());
    std::vector<uint8_t> g;
    guards = again.fetch(g) && guards;
    if (c.max_compressed_buffer_size != plain_cfg.max_compressed_buffer_size || fetch_size(d_bytes) != plain_bytes
        || *c.get_status() != *plain_cfg.get_status() || (plain_bytes <= h.size() && !std::equal(g.begin(), g.begin() + plain_bytes, h.begin())))
      plain_bytes = ~size_t(0) >> 1; // (reported: no stream is this long)
  }
  HIP(hipMemset(d_bytes, 0xEE, 8));
  hipcomp::CompressionConfig cfg = m.configure_frame_compression(data.size(), Index::Leading);
  Guarded frame(cfg.max_compressed_buffer_size, off);
  m.compress_frame(d_in, frame.at, cfg, d_bytes, Index::Leading);
  HIP(hipDeviceSynchronize());
  const int status = (int)*cfg.get_status();
  size_t frame_bytes = fetch_size(d_bytes);
  guards = frame.fetch(h) && guards;
  if (frame_bytes > h.size())
    frame_bytes = h.size() + 1; // (reported as it is wrong; nothing to write)
  else
    write_file(frame_path, h.data(), frame_bytes);
  int roundtrip = 0;
  long walked = -1;
  if (status == 0 && frame_bytes <= h.size()) {
    hipcomp::DecompressionConfig dcfg = m.configure_frame_decompression(frame.at, frame_bytes);
    if (*dcfg.get_status() == hipcompSuccess && dcfg.decomp_data_size == data.size()) {
      Guarded back(data.size(), off);
      m.decompress_frame(back.at, frame.at, frame_bytes, dcfg);
      HIP(hipDeviceSynchronize());
      walked = (long)m.get_frame_walked_chunks();
      std::vector<uint8_t> b;
      const bool ok = back.fetch(b);
      roundtrip = ok && *dcfg.get_status() == hipcompSuccess && b == data ? 1 : 0;
    }
  }
  std::printf("status %d frame_bytes %zu bound %zu plain_bytes %zu plain_bound %zu guards %d scratch_guard %d roundtrip %d walked %ld\n",
              status, frame_bytes, (size_t)cfg.max_compressed_buffer_size, plain_bytes, (size_t)plain_cfg.max_compressed_buffer_size,
              guards ? 1 : 0, scratch.intact() ? 1 : 0, roundtrip, walked);
  HIP(hipFree(d_in_base));
  HIP(hipFree(d_bytes));
}

// the file's bytes `off` bytes behind a 256-byte boundary, at the very end of their allocation
struct Input
{
  uint8_t* base = nullptr;
  uint8_t* at = nullptr;
  Input(const std::vector<uint8_t>& data, size_t off)
  {
    HIP(hipMalloc((void**)&base, 256 + off + data.size() + 1));
    HIP(hipMemset(base, 0x04, 256 + off + data.size() + 1));
    at = base + 256 + off;
    if (!data.empty())
      HIP(hipMemcpy(at, data.data(), data.size(), hipMemcpyHostToDevice));
  }
  ~Input() { (void)hipFree(base); }
};

static void read_one(std::istringstream& line, bool displaced)
{
  int policy = 0;
  size_t chunk = 0, off_in = 0, off_out = 0;
  std::string in_path, out_path, scratch_word;
  line >> chunk >> policy >> in_path >> out_path >> scratch_word >> off_in >> off_out;
  const std::vector<uint8_t> data = read_file(in_path);
  hipcomp::SnappyManager m(chunk, 0, 0, (hipcomp::ChecksumPolicy)policy);
  Scratch scratch;
  if (scratch_word == "scratch")
    scratch.give(m);
  Input in(data, off_in);
  hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(in.at, data.size());
  const int configured = (int)*cfg.get_status();
  Guarded out(cfg.decomp_data_size, off_out);
  const Input other(std::vector<uint8_t>(16, 0), 0); // (no stream at all: refused, and the last buffer configured)
  if (displaced)
    (void)m.configure_frame_decompression(other.at, 16);
  m.decompress_frame(out.at, in.at, data.size(), cfg);
  HIP(hipDeviceSynchronize());
  const long walked = (long)m.get_frame_walked_chunks();
  std::vector<uint8_t> h;
  const bool guards = out.fetch(h);
  write_file(out_path, h.data(), h.size());
  std::printf("configured %d status %d size %zu chunks %u guards %d scratch_guard %d walked %ld\n", configured,
              (int)*cfg.get_status(), (size_t)cfg.decomp_data_size, (unsigned)cfg.num_chunks, guards ? 1 : 0,
              scratch.intact() ? 1 : 0, walked);
}

static void range_one(std::istringstream& line)
{
  int policy = 0;
  size_t chunk = 0, off_in = 0, off_out = 0, first = 0, count = 0;
  std::string in_path, out_path, scratch_word;
  line >> chunk >> policy >> in_path >> out_path >> scratch_word >> off_in >> off_out >> first >> count;
  const std::vector<uint8_t> data = read_file(in_path);
  hipcomp::SnappyManager m(chunk, 0, 0, (hipcomp::ChecksumPolicy)policy);
  Scratch scratch;
  if (scratch_word == "scratch")
    scratch.give(m);
  Input in(data, off_in);
  hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(in.at, data.size());
  const int configured = (int)*cfg.get_status();
  Guarded out(count, off_out);
  m.decompress_frame_range(out.at, in.at, data.size(), cfg, first, count);
  HIP(hipDeviceSynchronize());
  std::vector<uint8_t> h;
  const bool guards = out.fetch(h);
  write_file(out_path, h.data(), h.size());
  const bool untouched = std::all_of(h.begin(), h.end(), [](uint8_t b) { return b == kGuardByte; });
  std::printf("configured %d status %d size %zu guards %d scratch_guard %d untouched %d walked %ld\n", configured,
              (int)*cfg.get_status(), (size_t)cfg.decomp_data_size, guards ? 1 : 0, scratch.intact() ? 1 : 0, untouched ? 1 : 0,
              (long)m.get_frame_walked_chunks());
}

static int limits()
{
  hipcomp::SnappyManager m(1, 0, 0, hipcomp::NoComputeNoVerify);
  const size_t most = 4194294;
  for (int k = 0; k < 3; ++k) {
    const size_t n = k == 0 ? most : most + 1;
    hipcomp::CompressionConfig c = m.configure_frame_compression(n, k == 2 ? Index::None : Index::Leading);
    std::printf("chunks %zu status %d bound %zu chunks_configured %zu\n", n, (int)*c.get_status(), (size_t)c.max_compressed_buffer_size,
                (size_t)c.num_chunks);
  }
  return 0;
}

// ---- timing (scripts/quick_snappy_frame_index.py) ------------------------------------------------------------
static std::vector<uint8_t> uniform_bytes(size_t n)
{
  std::vector<uint8_t> h(n + 8);
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (size_t i = 0; i < n; i += 8) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    std::memcpy(&h[i], &x, 8);
  }
  h.resize(n);
  return h;
}

// per policy: decompress_frame of the indexed stream, of the stream without an index, decompress of the container,
// decompress_frame_range of 1 MiB from the middle of the indexed stream -- they alternate inside every repetition; 2
// warm-up repetitions, medians of the rest.  The stream without an index is read twice: configured just before (the
// host knows it has no index and launches the chain's passes alone) and with another buffer configured in between
// (the indexed passes are launched and refuse on the device).  configure_frame_decompression synchronises, so it is
// timed by the host's clock.
static int timing(const char* data_path, size_t chunks, int reps)
{
  const size_t chunk = 65536;
  std::vector<uint8_t> data = data_path[0] == '-' ? uniform_bytes(chunks * chunk) : read_file(data_path);
  const size_t n = data.size();
  // (1 MiB from the middle, off every chunk boundary)
  const size_t range_bytes = n < (1u << 20) ? n : (1u << 20), range_first = (n - range_bytes) / 2 + (n > range_bytes + 8192 ? 1234 : 0);
  uint8_t *d_in = nullptr, *d_indexed = nullptr, *d_plain = nullptr, *d_cont = nullptr, *d_back = nullptr;
  size_t* d_bytes = nullptr;
  HIP(hipMalloc((void**)&d_in, n + 16));
  HIP(hipMalloc((void**)&d_back, n + 16));
  HIP(hipMalloc((void**)&d_bytes, 8));
  HIP(hipMemcpy(d_in, data.data(), n, hipMemcpyHostToDevice));
  hipEvent_t a, b;
  HIP(hipEventCreate(&a));
  HIP(hipEventCreate(&b));
  for (hipcomp::ChecksumPolicy p : {hipcomp::NoComputeNoVerify, hipcomp::ComputeAndVerify}) {
    hipcomp::SnappyManager m(chunk, 0, 0, p);
    hipcomp::CompressionConfig icfg = m.configure_frame_compression(n, Index::Leading), fcfg = m.configure_frame_compression(n),
                               ccfg = m.configure_compression(n);
    if (!d_indexed) {
      HIP(hipMalloc((void**)&d_indexed, icfg.max_compressed_buffer_size + 64));
      HIP(hipMalloc((void**)&d_plain, fcfg.max_compressed_buffer_size + 64));
      HIP(hipMalloc((void**)&d_cont, ccfg.max_compressed_buffer_size));
    }
    m.compress_frame(d_in, d_indexed, icfg, d_bytes, Index::Leading);
    HIP(hipDeviceSynchronize());
    const size_t indexed_bytes = fetch_size(d_bytes);
    m.compress_frame(d_in, d_plain, fcfg, d_bytes);
    m.compress(d_in, d_cont, ccfg);
    HIP(hipDeviceSynchronize());
    const size_t plain_bytes = fetch_size(d_bytes);
    hipcomp::DecompressionConfig id = m.configure_frame_decompression(d_indexed, indexed_bytes);
    hipcomp::DecompressionConfig rd = m.configure_frame_decompression(d_indexed, indexed_bytes);
    hipcomp::DecompressionConfig fd = m.configure_frame_decompression(d_plain, plain_bytes), cd = m.configure_decompression(ccfg);
    std::vector<std::vector<float>> ms(9);
    auto configure_ms = [&](hipcomp::DecompressionConfig& c, const uint8_t* p_, size_t n_) {
      HIP(hipDeviceSynchronize());
      const auto t0 = std::chrono::steady_clock::now();
      c = m.configure_frame_decompression(p_, n_);
      return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    int worst = 0;
    long walked[3] = {-1, -1, -1};
    for (int r = 0; r < reps + 2; ++r)
      for (int k = 0; k < 7; ++k) {
        float t = 0, c = 0;
        // (the hint of the last configure call is the plain stream's: the indexed stream is read without one, the
        // plain one with it, as a caller that configures before every read has it)
        if (k == 1)
          c = configure_ms(fd, d_plain, plain_bytes);
        if (k == 5) // (the last buffer configured is the indexed one: the plain one is read without the host's word)
          c = configure_ms(id, d_indexed, indexed_bytes);
        HIP(hipEventRecord(a, 0));
        if (k == 0)
          m.decompress_frame(d_back, d_indexed, indexed_bytes, id);
        else if (k == 1 || k == 5)
          m.decompress_frame(d_back, d_plain, plain_bytes, fd);
        else if (k == 2)
          m.decompress(d_back, d_cont, cd);
        else if (k == 3)
          m.compress_frame(d_in, d_indexed, icfg, d_bytes, Index::Leading);
        else if (k == 4)
          m.compress_frame(d_in, d_plain, fcfg, d_bytes);
        else if (k == 6)
          m.decompress_frame_range(d_back, d_indexed, indexed_bytes, rd, range_first, range_bytes);
        HIP(hipEventRecord(b, 0));
        HIP(hipEventSynchronize(b));
        HIP(hipEventElapsedTime(&t, a, b));
        if (k < 2)
          walked[k] = (long)m.get_frame_walked_chunks();
        if (k == 5)
          walked[2] = (long)m.get_frame_walked_chunks();
        worst = std::max({worst, (int)*id.get_status(), (int)*fd.get_status(), (int)*cd.get_status(), (int)*icfg.get_status(),
                          (int)*fcfg.get_status(), (int)*rd.get_status()});
        if (r >= 2) {
          ms[k == 6 ? 8 : k].push_back(t);
          if (k == 1)
            ms[6].push_back(c);
          if (k == 5)
            ms[7].push_back(c);
        }
      }
    for (auto& v : ms)
      std::sort(v.begin(), v.end());
    auto med = [&](int k) { return ms[k][ms[k].size() / 2]; };
    std::printf("policy %d decompress_frame_indexed median_ms %.4f decompress_frame_plain median_ms %.4f decompress median_ms %.4f\n",
                (int)p, med(0), med(1), med(2));
    std::printf("policy %d decompress_frame_plain_displaced median_ms %.4f configure_plain median_ms %.4f configure_indexed median_ms %.4f\n",
                (int)p, med(5), med(6), med(7));
    std::printf("policy %d compress_frame_indexed median_ms %.4f compress_frame_plain median_ms %.4f decompress_frame_range_1mib median_ms %.4f\n",
                (int)p, med(3), med(4), med(8));
    std::printf("policy %d bytes %zu indexed_bytes %zu plain_bytes %zu walked_indexed %ld walked_plain %ld walked_plain_displaced %ld worst_status %d\n",
                (int)p, n, indexed_bytes, plain_bytes, walked[0], walked[1], walked[2], worst);
  }
  return 0;
}

// compress_frame, compress, decompress_frame, decompress of the same data without an index, alternating, as
// tests/snappy_frame_driver.cpp times them
static int timing_plain(const char* data_path, size_t chunks, int reps, bool displaced)
{
  const size_t chunk = 65536;
  std::vector<uint8_t> data = data_path[0] == '-' ? uniform_bytes(chunks * chunk) : read_file(data_path);
  const size_t n = data.size();
  uint8_t *d_in = nullptr, *d_frame = nullptr, *d_cont = nullptr, *d_back = nullptr;
  size_t* d_bytes = nullptr;
  HIP(hipMalloc((void**)&d_in, n + 16));
  HIP(hipMalloc((void**)&d_back, n + 16));
  HIP(hipMalloc((void**)&d_bytes, 8));
  HIP(hipMemcpy(d_in, data.data(), n, hipMemcpyHostToDevice));
  const Input other(std::vector<uint8_t>(16, 0), 0);
  hipEvent_t a, b;
  HIP(hipEventCreate(&a));
  HIP(hipEventCreate(&b));
  for (hipcomp::ChecksumPolicy p : {hipcomp::NoComputeNoVerify, hipcomp::ComputeAndVerify}) {
    hipcomp::SnappyManager m(chunk, 0, 0, p);
    hipcomp::CompressionConfig fcfg = m.configure_frame_compression(n), ccfg = m.configure_compression(n);
    if (!d_frame) {
      HIP(hipMalloc((void**)&d_frame, fcfg.max_compressed_buffer_size + 64));
      HIP(hipMalloc((void**)&d_cont, ccfg.max_compressed_buffer_size));
    }
    m.compress_frame(d_in, d_frame, fcfg, d_bytes);
    m.compress(d_in, d_cont, ccfg);
    HIP(hipDeviceSynchronize());
    const size_t frame_bytes = fetch_size(d_bytes);
    hipcomp::DecompressionConfig fd = m.configure_frame_decompression(d_frame, frame_bytes), cd = m.configure_decompression(ccfg);
    if (displaced)
      (void)m.configure_frame_decompression(other.at, 16);
    std::vector<std::vector<float>> ms(4);
    int worst = 0;
    long walked = -1;
    for (int r = 0; r < reps + 2; ++r)
      for (int k = 0; k < 4; ++k) {
        float t = 0;
        HIP(hipEventRecord(a, 0));
        if (k == 0)
          m.compress_frame(d_in, d_frame, fcfg, d_bytes);
        else if (k == 1)
          m.compress(d_in, d_cont, ccfg);
        else if (k == 2)
          m.decompress_frame(d_back, d_frame, frame_bytes, fd);
        else
          m.decompress(d_back, d_cont, cd);
        HIP(hipEventRecord(b, 0));
        HIP(hipEventSynchronize(b));
        HIP(hipEventElapsedTime(&t, a, b));
        worst = std::max({worst, (int)*fcfg.get_status(), (int)*ccfg.get_status(), (int)*fd.get_status(), (int)*cd.get_status()});
        if (r >= 2)
          ms[k].push_back(t);
        if (r == reps + 1 && k == 2)
          walked = (long)m.get_frame_walked_chunks();
      }
    for (auto& v : ms)
      std::sort(v.begin(), v.end());
    std::printf("policy %d decompress_frame_plain_%s median_ms %.4f min_ms %.4f max_ms %.4f decompress median_ms %.4f compress_frame median_ms %.4f walked %ld worst_status %d\n",
                (int)p, displaced ? "displaced" : "configured", ms[2][ms[2].size() / 2], ms[2].front(), ms[2].back(),
                ms[3][ms[3].size() / 2], ms[0][ms[0].size() / 2], walked, worst);
  }
  return 0;
}

int main(int argc, char** argv)
{
  try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if ((cmd == "write" || cmd == "read" || cmd == "read_displaced" || cmd == "range") && argc == 3) {
      std::ifstream list(argv[2]);
      std::string text;
      while (std::getline(list, text)) {
        if (text.empty())
          continue;
        std::istringstream line(text);
        if (cmd == "write")
          write_one(line);
        else if (cmd == "read" || cmd == "read_displaced")
          read_one(line, cmd == "read_displaced");
        else
          range_one(line);
        std::fflush(stdout);
      }
      return 0;
    }
    if (cmd == "limits" && argc == 2)
      return limits();
    if (cmd == "timing" && argc == 5)
      return timing(argv[2], std::strtoull(argv[3], nullptr, 0), std::atoi(argv[4]));
    if (cmd == "timing_plain" && argc == 6)
      return timing_plain(argv[2], std::strtoull(argv[3], nullptr, 0), std::atoi(argv[4]), std::string(argv[5]) == "displaced");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 4;
  }
  std::fprintf(stderr, "usage: see the head of snappy_frame_index_driver.cpp\n");
  return 2;
}
