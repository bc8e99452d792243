// The Snappy manager's framed-stream methods (hipcomp/snappy.hpp: compress_frame, decompress_frame and their configure
// calls) driven on files, for tests/test_snappy_frame_gpu.py and scripts/quick_snappy_frame.py.  Written against
// include/ and linked to libhipcomp.so.
//   snappy_frame_driver write LIST
//       every line of LIST: CHUNK POLICY IN FRAME BLOCKS scratch|own OFF
//       A manager of CHUNK-byte chunks with the ChecksumPolicy POLICY compresses the file IN (placed OFF bytes behind a
//       256-byte boundary) to one stream, written OFF bytes behind a 256-byte boundary between guard bytes into a
//       buffer of exactly max_compressed_buffer_size bytes; FRAME gets the frame_bytes bytes.  BLOCKS gets what
//       hipcompBatchedSnappyCompressAsync writes for the same chunks: per chunk a u64 size and the bytes.  Then the
//       stream is read back by decompress_frame under managers of each of the five policies.  scratch: caller-owned
//       scratch buffers of exactly get_required_scratch_buffer_size() bytes with guard bytes behind them.
//       prints "status S frame_bytes F bound B guards G scratch_guard H roundtrip R"
//       (R: bit p set = decompress_frame under policy p gave status 0 and the input back between intact guards)
//   snappy_frame_driver read LIST
//       every line of LIST: POLICY IN OUT scratch|own OFF_IN OFF_OUT TAIL
//       configure_frame_decompression + decompress_frame of the file IN (OFF_IN bytes behind a 256-byte boundary;
//       behind it the bytes of the file TAIL, then zeros; TAIL "-": bytes 0x04, which no reader may take) into a buffer
//       of exactly decomp_data_size bytes OFF_OUT bytes behind a 256-byte boundary between guard bytes; OUT gets those.
//       prints "configured C status S size D chunks N guards G scratch_guard H" (C: the status after configure)
//   snappy_frame_driver timing DATA|- CHUNKS REPS
//   snappy_frame_driver timing_read FRAME REPS
//       see scripts/quick_snappy_frame.py
#include "hipcomp/snappy.h"
#include "hipcomp/snappy.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
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

// what the batched API writes for the chunks of d_in: per chunk a u64 size and the bytes
static std::vector<uint8_t> batched_blocks(const uint8_t* d_in, size_t n, size_t chunk)
{
  const size_t count = (n + chunk - 1) / chunk;
  std::vector<uint8_t> out;
  if (count == 0)
    return out;
  const hipcompBatchedSnappyOpts_t opts = hipcompBatchedSnappyDefaultOpts;
  size_t temp_bytes = 0, slot = 0;
  if (hipcompBatchedSnappyCompressGetTempSize(count, chunk, opts, &temp_bytes) != hipcompSuccess
      || hipcompBatchedSnappyCompressGetMaxOutputChunkSize(chunk, opts, &slot) != hipcompSuccess)
    std::exit(5);
  std::vector<const void*> in_ptrs(count);
  std::vector<size_t> in_bytes(count);
  std::vector<void*> out_ptrs(count);
  uint8_t *d_slots = nullptr, *d_temp = nullptr, *d_lists = nullptr;
  HIP(hipMalloc((void**)&d_slots, count * slot));
  HIP(hipMalloc((void**)&d_temp, temp_bytes + 16));
  HIP(hipMalloc((void**)&d_lists, count * 32));
  for (size_t i = 0; i < count; ++i) {
    in_ptrs[i] = d_in + i * chunk;
    in_bytes[i] = std::min(chunk, n - i * chunk);
    out_ptrs[i] = d_slots + i * slot;
  }
  HIP(hipMemcpy(d_lists, in_ptrs.data(), count * 8, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_lists + count * 8, in_bytes.data(), count * 8, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_lists + count * 16, out_ptrs.data(), count * 8, hipMemcpyHostToDevice));
  if (hipcompBatchedSnappyCompressAsync((const void* const*)d_lists, (const size_t*)(d_lists + count * 8), chunk, count, d_temp,
                                        temp_bytes, (void* const*)(d_lists + count * 16), (size_t*)(d_lists + count * 24), opts, 0)
      != hipcompSuccess)
    std::exit(5);
  HIP(hipDeviceSynchronize());
  std::vector<size_t> sizes(count);
  HIP(hipMemcpy(sizes.data(), d_lists + count * 24, count * 8, hipMemcpyDeviceToHost));
  std::vector<uint8_t> slots(count * slot);
  HIP(hipMemcpy(slots.data(), d_slots, slots.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < count; ++i) {
    const uint64_t s = sizes[i];
    out.insert(out.end(), (const uint8_t*)&s, (const uint8_t*)&s + 8);
    out.insert(out.end(), slots.begin() + i * slot, slots.begin() + i * slot + s);
  }
  HIP(hipFree(d_slots));
  HIP(hipFree(d_temp));
  HIP(hipFree(d_lists));
  return out;
}

static void write_one(std::istringstream& line)
{
  size_t chunk = 0, off = 0;
  int policy = 0;
  std::string in_path, frame_path, blocks_path, scratch_word;
  line >> chunk >> policy >> in_path >> frame_path >> blocks_path >> scratch_word >> off;
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
  hipcomp::CompressionConfig cfg = m.configure_frame_compression(data.size());
  Guarded frame(cfg.max_compressed_buffer_size, off);
  m.compress_frame(d_in, frame.at, cfg, d_bytes);
  HIP(hipDeviceSynchronize());
  const int status = (int)*cfg.get_status();
  size_t frame_bytes = 0;
  HIP(hipMemcpy(&frame_bytes, d_bytes, 8, hipMemcpyDeviceToHost));
  std::vector<uint8_t> h;
  const bool guards = frame.fetch(h);
  if (frame_bytes > h.size())
    frame_bytes = h.size() + 1; // (reported as it is wrong; nothing to write)
  else
    write_file(frame_path, h.data(), frame_bytes);
  bool scratch_ok = scratch.intact();
  int roundtrip = 0;
  if (status == 0 && frame_bytes <= h.size()) {
    const std::vector<uint8_t> blocks = batched_blocks(d_in, data.size(), chunk);
    write_file(blocks_path, blocks.data(), blocks.size());
    for (int p = 0; p < 5; ++p) {
      hipcomp::SnappyManager r(chunk, 0, 0, (hipcomp::ChecksumPolicy)p);
      Scratch rs;
      if (scratch_word == "scratch")
        rs.give(r);
      hipcomp::DecompressionConfig dcfg = r.configure_frame_decompression(frame.at, frame_bytes);
      if (*dcfg.get_status() != hipcompSuccess || dcfg.decomp_data_size != data.size())
        continue;
      Guarded back(data.size(), off);
      r.decompress_frame(back.at, frame.at, frame_bytes, dcfg);
      HIP(hipDeviceSynchronize());
      std::vector<uint8_t> b;
      const bool ok = back.fetch(b);
      if (ok && *dcfg.get_status() == hipcompSuccess && b == data)
        roundtrip |= 1 << p;
      scratch_ok = scratch_ok && rs.intact();
    }
  }
  std::printf("status %d frame_bytes %zu bound %zu guards %d scratch_guard %d roundtrip %d\n", status, frame_bytes,
              (size_t)cfg.max_compressed_buffer_size, guards ? 1 : 0, scratch_ok ? 1 : 0, roundtrip);
  HIP(hipFree(d_in_base));
  HIP(hipFree(d_bytes));
}

static void read_one(std::istringstream& line)
{
  int policy = 0;
  size_t off_in = 0, off_out = 0;
  std::string in_path, out_path, scratch_word, tail_path;
  line >> policy >> in_path >> out_path >> scratch_word >> off_in >> off_out >> tail_path;
  const std::vector<uint8_t> data = read_file(in_path);
  hipcomp::SnappyManager m(65536, 0, 0, (hipcomp::ChecksumPolicy)policy);
  Scratch scratch;
  if (scratch_word == "scratch")
    scratch.give(m);
  // the input inside a larger buffer: what stands behind frames_bytes must change nothing
  uint8_t* d_in_base = nullptr;
  HIP(hipMalloc((void**)&d_in_base, data.size() + 1024));
  uint8_t* const d_in = d_in_base + 256 + off_in;
  if (tail_path == "-") {
    HIP(hipMemset(d_in_base, 0x04, data.size() + 1024));
  } else {
    HIP(hipMemset(d_in_base, 0, data.size() + 1024));
    const std::vector<uint8_t> tail = read_file(tail_path);
    if (tail.size() > 512)
      std::exit(2);
    if (!tail.empty())
      HIP(hipMemcpy(d_in + data.size(), tail.data(), tail.size(), hipMemcpyHostToDevice));
  }
  if (!data.empty())
    HIP(hipMemcpy(d_in, data.data(), data.size(), hipMemcpyHostToDevice));
  hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(d_in, data.size());
  const int configured = (int)*cfg.get_status();
  Guarded out(cfg.decomp_data_size, off_out);
  m.decompress_frame(out.at, d_in, data.size(), cfg);
  HIP(hipDeviceSynchronize());
  std::vector<uint8_t> h;
  const bool guards = out.fetch(h);
  write_file(out_path, h.data(), h.size());
  std::printf("configured %d status %d size %zu chunks %u guards %d scratch_guard %d\n", configured, (int)*cfg.get_status(),
              (size_t)cfg.decomp_data_size, (unsigned)cfg.num_chunks, guards ? 1 : 0, scratch.intact() ? 1 : 0);
  HIP(hipFree(d_in_base));
}

// ---- timing (scripts/quick_snappy_frame.py) ------------------------------------------------------------------
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

// rows: name, milliseconds of the framed call and of the container call it is compared with
static int timing(const char* data_path, size_t chunks, int reps)
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
    size_t frame_bytes = 0;
    HIP(hipMemcpy(&frame_bytes, d_bytes, 8, hipMemcpyDeviceToHost));
    hipcomp::DecompressionConfig fd = m.configure_frame_decompression(d_frame, frame_bytes), cd = m.configure_decompression(ccfg);
    std::vector<std::vector<float>> ms(4);
    int worst = 0;
    // the calls alternate inside every repetition; 2 warm-up repetitions
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
      }
    for (auto& v : ms)
      std::sort(v.begin(), v.end());
    std::printf("policy %d compress_frame median_ms %.4f compress median_ms %.4f\n", (int)p, ms[0][ms[0].size() / 2],
                ms[1][ms[1].size() / 2]);
    std::printf("policy %d decompress_frame median_ms %.4f decompress median_ms %.4f\n", (int)p, ms[2][ms[2].size() / 2],
                ms[3][ms[3].size() / 2]);
    std::printf("policy %d bytes %zu frame_bytes %zu chunks %u worst_status %d\n", (int)p, n, frame_bytes, (unsigned)fd.num_chunks,
                worst);
  }
  return 0;
}

// one stream file read `reps` times under a non-verifying and a verifying policy
static int timing_read(const char* frame_path, int reps)
{
  const std::vector<uint8_t> f = read_file(frame_path);
  uint8_t* d_frame = nullptr;
  HIP(hipMalloc((void**)&d_frame, f.size() + 16));
  HIP(hipMemcpy(d_frame, f.data(), f.size(), hipMemcpyHostToDevice));
  hipEvent_t a, b;
  HIP(hipEventCreate(&a));
  HIP(hipEventCreate(&b));
  for (hipcomp::ChecksumPolicy p : {hipcomp::NoComputeNoVerify, hipcomp::ComputeAndVerify}) {
    hipcomp::SnappyManager m(65536, 0, 0, p);
    hipcomp::DecompressionConfig cfg = m.configure_frame_decompression(d_frame, f.size());
    uint8_t* d_out = nullptr;
    HIP(hipMalloc((void**)&d_out, cfg.decomp_data_size + 16));
    std::vector<float> ms;
    for (int r = 0; r < reps + 2; ++r) {
      float t = 0;
      HIP(hipEventRecord(a, 0));
      m.decompress_frame(d_out, d_frame, f.size(), cfg);
      HIP(hipEventRecord(b, 0));
      HIP(hipEventSynchronize(b));
      HIP(hipEventElapsedTime(&t, a, b));
      if (r >= 2)
        ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    std::printf("policy %d decompress_frame median_ms %.4f bytes %zu chunks %u status %d\n", (int)p, ms[ms.size() / 2],
                (size_t)cfg.decomp_data_size, (unsigned)cfg.num_chunks, (int)*cfg.get_status());
    HIP(hipFree(d_out));
  }
  return 0;
}

int main(int argc, char** argv)
{
  try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if ((cmd == "write" || cmd == "read") && argc == 3) {
      std::ifstream list(argv[2]);
      std::string text;
      while (std::getline(list, text)) {
        if (text.empty())
          continue;
        std::istringstream line(text);
        if (cmd == "write")
          write_one(line);
        else
          read_one(line);
        std::fflush(stdout);
      }
      return 0;
    }
    if (cmd == "timing" && argc == 5)
      return timing(argv[2], std::strtoull(argv[3], nullptr, 0), std::atoi(argv[4]));
    if (cmd == "timing_read" && argc == 4)
      return timing_read(argv[2], std::atoi(argv[3]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 4;
  }
  std::fprintf(stderr, "usage: see the head of snappy_frame_driver.cpp\n");
  return 2;
}
