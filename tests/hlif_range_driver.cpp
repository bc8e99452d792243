// Ranged reads of the high-level managers (hipcomp/hipcompManager.hpp, decompress_range) driven on files, for
// tests/test_hlif_range_gpu.py and scripts/quick_range.py.  Written against include/ and linked to libhipcomp.so.
//   hlif_range_driver compress CODEC POLICY IN OUT
//       CODEC: lz4:CHUNK:TYPE | snappy:CHUNK | cascaded:CHUNK:TYPE:RLES:DELTAS:BP
//       POLICY: 0..4 (the ChecksumPolicy) or "old" (the constructor without a policy); prints "status S"
//   hlif_range_driver range CODEC POLICY CONTAINER OUT first_byte num_bytes [out_misalign] [scratch] [full]
//                           [poke=AT:XOR ...]
//       the manager of CODEC with the policy; configure_decompression(container), then every poke (byte AT of the
//       container on the device ^= XOR: a header that changes behind the configuration's back), then
//       decompress_range into a buffer that lies out_misalign bytes off a 256-byte boundary between 64 guard bytes on
//       each side; OUT gets out[0, num_bytes).  scratch: a caller-owned scratch buffer of exactly
//       get_required_scratch_buffer_size() bytes with 256 guard bytes behind it.  full: also decompress() the
//       container and compare its bytes [first_byte, first_byte + num_bytes) with the ranged read's.
//       prints "status S guards G scratch_guard H size D [same_as_decompress E]" (G, H: 1 = intact)
//   hlif_range_driver timing CHUNKS REPS
//       the LZ4 manager, CHUNKS x 64 KiB uniform random bytes: decompress against decompress_range of 1 byte, one
//       chunk's worth, 1 % and 50 % of the buffer (none aligned to chunks), NoComputeNoVerify and ComputeAndVerify,
//       milliseconds per call by HIP events (median and minimum of REPS)
#include "hipcomp/hipcompManagerFactory.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static std::vector<uint8_t> read_file(const char* path)
{
  FILE* f = std::fopen(path, "rb");
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

static void write_file(const char* path, const uint8_t* p, size_t n)
{
  FILE* f = std::fopen(path, "wb");
  if (!f || (n && std::fwrite(p, 1, n, f) != n))
    std::exit(2);
  std::fclose(f);
}

static std::vector<std::string> split(const std::string& s)
{
  std::vector<std::string> out;
  size_t at = 0, c;
  while ((c = s.find(':', at)) != std::string::npos) {
    out.push_back(s.substr(at, c - at));
    at = c + 1;
  }
  out.push_back(s.substr(at));
  return out;
}

// one of the three managers: decompress_range is a member of each, not of their base
struct Manager
{
  std::unique_ptr<hipcomp::LZ4Manager> lz4;
  std::unique_ptr<hipcomp::SnappyManager> snappy;
  std::unique_ptr<hipcomp::CascadedManager> cascaded;
  hipcomp::hipcompManagerBase& base()
  {
    return lz4 ? static_cast<hipcomp::hipcompManagerBase&>(*lz4)
               : snappy ? static_cast<hipcomp::hipcompManagerBase&>(*snappy) : *cascaded;
  }
  void decompress_range(uint8_t* out, const uint8_t* comp, const hipcomp::DecompressionConfig& cfg, size_t first, size_t n)
  {
    if (lz4)
      lz4->decompress_range(out, comp, cfg, first, n);
    else if (snappy)
      snappy->decompress_range(out, comp, cfg, first, n);
    else
      cascaded->decompress_range(out, comp, cfg, first, n);
  }
};

static Manager make_manager(const std::string& codec, const std::string& policy)
{
  const std::vector<std::string> f = split(codec);
  const bool old = policy == "old";
  const hipcomp::ChecksumPolicy p = old ? hipcomp::NoComputeNoVerify : (hipcomp::ChecksumPolicy)std::atoi(policy.c_str());
  const size_t chunk = std::strtoull(f.at(1).c_str(), nullptr, 0);
  Manager m;
  if (f[0] == "lz4") {
    const hipcompType_t t = (hipcompType_t)std::atoi(f.at(2).c_str());
    m.lz4.reset(old ? new hipcomp::LZ4Manager(chunk, t) : new hipcomp::LZ4Manager(chunk, t, 0, 0, p));
  } else if (f[0] == "snappy") {
    m.snappy.reset(old ? new hipcomp::SnappyManager(chunk) : new hipcomp::SnappyManager(chunk, 0, 0, p));
  } else {
    hipcompBatchedCascadedOpts_t o = hipcompBatchedCascadedDefaultOpts;
    o.chunk_size = chunk;
    o.type = (hipcompType_t)std::atoi(f.at(2).c_str());
    o.num_RLEs = std::atoi(f.at(3).c_str());
    o.num_deltas = std::atoi(f.at(4).c_str());
    o.use_bp = std::atoi(f.at(5).c_str());
    m.cascaded.reset(old ? new hipcomp::CascadedManager(o) : new hipcomp::CascadedManager(o, 0, 0, p));
  }
  return m;
}

static int compress(const std::string& codec, const std::string& policy, const char* in, const char* out)
{
  const std::vector<uint8_t> data = read_file(in);
  Manager m = make_manager(codec, policy);
  uint8_t *d_in = nullptr, *d_out = nullptr;
  HIP(hipMalloc((void**)&d_in, data.size() + 16));
  if (!data.empty())
    HIP(hipMemcpy(d_in, data.data(), data.size(), hipMemcpyHostToDevice));
  hipcomp::CompressionConfig cfg = m.base().configure_compression(data.size());
  HIP(hipMalloc((void**)&d_out, cfg.max_compressed_buffer_size));
  m.base().compress(d_in, d_out, cfg);
  HIP(hipDeviceSynchronize());
  const size_t bytes = m.base().get_compressed_output_size(d_out);
  std::vector<uint8_t> c(bytes);
  HIP(hipMemcpy(c.data(), d_out, bytes, hipMemcpyDeviceToHost));
  write_file(out, c.data(), bytes);
  std::printf("status %d\n", (int)*cfg.get_status());
  m = Manager();
  HIP(hipFree(d_in));
  HIP(hipFree(d_out));
  return 0;
}

constexpr size_t kGuard = 64, kScratchGuard = 256;
constexpr uint8_t kGuardByte = 0xA5, kScratchGuardByte = 0x5C;

static int range(int argc, char** argv)
{
  const std::string codec = argv[2], policy = argv[3];
  const std::vector<uint8_t> c = read_file(argv[4]);
  const char* out_path = argv[5];
  const size_t first = std::strtoull(argv[6], nullptr, 0), num = std::strtoull(argv[7], nullptr, 0);
  size_t misalign = 0;
  bool scratch = false, full = false;
  std::vector<std::pair<size_t, unsigned>> pokes;
  for (int i = 8; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "scratch")
      scratch = true;
    else if (a == "full")
      full = true;
    else if (a.rfind("poke=", 0) == 0) {
      const std::vector<std::string> f = split(a.substr(5));
      pokes.emplace_back(std::strtoull(f.at(0).c_str(), nullptr, 0), (unsigned)std::strtoul(f.at(1).c_str(), nullptr, 0));
    } else
      misalign = std::strtoull(a.c_str(), nullptr, 0);
  }
  uint8_t* d_in = nullptr;
  HIP(hipMalloc((void**)&d_in, c.size() + 128));
  HIP(hipMemcpy(d_in, c.data(), c.size(), hipMemcpyHostToDevice));
  Manager m = make_manager(codec, policy);
  uint8_t* s = nullptr;
  size_t scratch_bytes = 0;
  if (scratch) {
    scratch_bytes = m.base().get_required_scratch_buffer_size();
    HIP(hipMalloc((void**)&s, scratch_bytes + kScratchGuard));
    HIP(hipMemset(s + scratch_bytes, kScratchGuardByte, kScratchGuard));
    m.base().set_scratch_buffer(s);
  }
  hipcomp::DecompressionConfig cfg = m.base().configure_decompression(d_in);
  for (const auto& p : pokes) {
    uint8_t b = 0;
    HIP(hipMemcpy(&b, d_in + p.first, 1, hipMemcpyDeviceToHost));
    b ^= (uint8_t)p.second;
    HIP(hipMemcpy(d_in + p.first, &b, 1, hipMemcpyHostToDevice));
  }
  // (a range the call must refuse gets no room at all: guard bytes only)
  const size_t room = first <= cfg.decomp_data_size && num <= cfg.decomp_data_size - first ? num : 0;
  const size_t total = 256 + kGuard + room + kGuard;
  uint8_t* d_buf = nullptr;
  HIP(hipMalloc((void**)&d_buf, total));
  HIP(hipMemset(d_buf, kGuardByte, total));
  uint8_t* const d_out = d_buf + kGuard + (256 - kGuard) + misalign; // misalign bytes behind a 256-byte boundary
  m.decompress_range(d_out, d_in, cfg, first, num);
  HIP(hipDeviceSynchronize());
  const int status = (int)*cfg.get_status();
  std::vector<uint8_t> h(total);
  HIP(hipMemcpy(h.data(), d_buf, total, hipMemcpyDeviceToHost));
  const size_t at = (size_t)(d_out - d_buf);
  bool guards = true;
  for (size_t i = 0; i < total; ++i)
    if ((i < at || i >= at + room) && h[i] != kGuardByte)
      guards = false;
  write_file(out_path, h.data() + at, room);
  bool scratch_guard = true;
  if (s) {
    std::vector<uint8_t> g(kScratchGuard);
    HIP(hipMemcpy(g.data(), s + scratch_bytes, kScratchGuard, hipMemcpyDeviceToHost));
    for (uint8_t b : g)
      scratch_guard = scratch_guard && b == kScratchGuardByte;
  }
  std::printf("status %d guards %d scratch_guard %d size %zu", status, guards ? 1 : 0, scratch_guard ? 1 : 0,
              (size_t)cfg.decomp_data_size);
  if (full) {
    uint8_t* d_all = nullptr;
    HIP(hipMalloc((void**)&d_all, cfg.decomp_data_size + 16));
    hipcomp::DecompressionConfig cfg2 = m.base().configure_decompression(d_in);
    m.base().decompress(d_all, d_in, cfg2);
    HIP(hipDeviceSynchronize());
    std::vector<uint8_t> all(cfg.decomp_data_size);
    if (!all.empty())
      HIP(hipMemcpy(all.data(), d_all, all.size(), hipMemcpyDeviceToHost));
    const bool same = *cfg2.get_status() == hipcompSuccess && status == 0 && first + room <= all.size()
                      && std::memcmp(all.data() + first, h.data() + at, room) == 0;
    std::printf(" same_as_decompress %d", same ? 1 : 0);
    HIP(hipFree(d_all));
  }
  std::printf("\n");
  m = Manager();
  HIP(hipFree(d_in));
  HIP(hipFree(d_buf));
  if (s)
    HIP(hipFree(s));
  return 0;
}

static int timing(size_t chunks, int reps)
{
  const size_t chunk = 65536, n = chunks * chunk;
  uint8_t *d_in = nullptr, *d_out = nullptr, *d_back = nullptr;
  HIP(hipMalloc((void**)&d_in, n));
  HIP(hipMalloc((void**)&d_back, n + 64));
  {
    std::vector<uint8_t> h(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n; i += 8) {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      std::memcpy(&h[i], &x, 8);
    }
    HIP(hipMemcpy(d_in, h.data(), n, hipMemcpyHostToDevice));
  }
  hipEvent_t a, b;
  HIP(hipEventCreate(&a));
  HIP(hipEventCreate(&b));
  // (first byte, bytes): none of them aligned to chunks, out one byte off a 16-byte boundary
  struct R { const char* name; size_t first, bytes; };
  const size_t off = 12345;
  const R ranges[] = {{"1_byte", (chunks / 3) * chunk + off, 1},
                      {"1_chunk", (chunks / 3) * chunk + off, chunk},
                      {"1_percent", (chunks / 3) * chunk + off, n / 100 + 1},
                      {"50_percent", (chunks / 4) * chunk + off, n / 2 + 1}};
  for (hipcomp::ChecksumPolicy p : {hipcomp::NoComputeNoVerify, hipcomp::ComputeAndVerify}) {
    hipcomp::LZ4Manager m(chunk, HIPCOMP_TYPE_CHAR, 0, 0, p);
    hipcomp::CompressionConfig cfg = m.configure_compression(n);
    if (!d_out)
      HIP(hipMalloc((void**)&d_out, cfg.max_compressed_buffer_size));
    m.compress(d_in, d_out, cfg);
    HIP(hipDeviceSynchronize());
    hipcomp::DecompressionConfig dcfg = m.configure_decompression(cfg);
    // the calls alternate inside every repetition (the first repetition: warm-up)
    std::vector<std::vector<float>> ms(5);
    int worst = 0;
    for (int r = 0; r < reps + 1; ++r) {
      for (int k = 0; k < 5; ++k) {
        float t = 0;
        HIP(hipEventRecord(a, 0));
        if (k == 0)
          m.decompress(d_back, d_out, dcfg);
        else
          m.decompress_range(d_back + 1, d_out, dcfg, ranges[k - 1].first, ranges[k - 1].bytes);
        HIP(hipEventRecord(b, 0));
        HIP(hipEventSynchronize(b));
        HIP(hipEventElapsedTime(&t, a, b));
        worst = std::max(worst, (int)*dcfg.get_status());
        if (r)
          ms[k].push_back(t);
      }
    }
    for (int k = 0; k < 5; ++k) {
      std::sort(ms[k].begin(), ms[k].end());
      std::printf("policy %d %-10s bytes %12zu median_ms %.4f min_ms %.4f\n", (int)p, k ? ranges[k - 1].name : "decompress",
                  k ? ranges[k - 1].bytes : n, ms[k][ms[k].size() / 2], ms[k][0]);
    }
    std::printf("policy %d worst_status %d\n", (int)p, worst);
  }
  HIP(hipFree(d_in));
  HIP(hipFree(d_out));
  HIP(hipFree(d_back));
  return 0;
}

int main(int argc, char** argv)
{
  try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "compress" && argc == 6)
      return compress(argv[2], argv[3], argv[4], argv[5]);
    if (cmd == "range" && argc >= 8)
      return range(argc, argv);
    if (cmd == "timing" && argc == 4)
      return timing(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 4;
  }
  std::fprintf(stderr, "usage: see the head of hlif_range_driver.cpp\n");
  return 2;
}
