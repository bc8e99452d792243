// The high-level managers' CRC-32 checksums (hipcomp/hipcompManager.hpp, ChecksumPolicy) driven on files, for
// tests/test_hlif_checksums_gpu.py.  Written against include/ and linked to libhipcomp.so.
//   hlif_checksum_driver compress CODEC POLICY IN OUT [scratch]
//       CODEC: lz4:CHUNK:TYPE | snappy:CHUNK | cascaded:CHUNK:TYPE:RLES:DELTAS:BP
//       POLICY: 0..4 (the ChecksumPolicy) or "old" (the constructor without a policy)
//       scratch: a caller-owned scratch buffer of get_required_scratch_buffer_size() bytes
//       prints "status S scratch B"
//   hlif_checksum_driver decompress POLICY IN OUT [scratch]
//       the manager from create_manager (with the policy, or the old overload for "old"); prints "status S"
//   hlif_checksum_driver timing CHUNKS REPS
//       the LZ4 manager, CHUNKS x 64 KiB uniform random bytes: compress and decompress, NoComputeNoVerify
//       against ComputeAndVerify, milliseconds per call by HIP events
#include "hipcomp/hipcompManagerFactory.hpp"

#include <hip/hip_runtime.h>

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

static std::unique_ptr<hipcomp::hipcompManagerBase> make_manager(const std::string& codec, const std::string& policy)
{
  const std::vector<std::string> f = split(codec);
  const bool old = policy == "old";
  const hipcomp::ChecksumPolicy p = old ? hipcomp::NoComputeNoVerify : (hipcomp::ChecksumPolicy)std::atoi(policy.c_str());
  const size_t chunk = std::strtoull(f.at(1).c_str(), nullptr, 0);
  if (f[0] == "lz4") {
    const hipcompType_t t = (hipcompType_t)std::atoi(f.at(2).c_str());
    if (old)
      return std::unique_ptr<hipcomp::hipcompManagerBase>(new hipcomp::LZ4Manager(chunk, t));
    return std::unique_ptr<hipcomp::hipcompManagerBase>(new hipcomp::LZ4Manager(chunk, t, 0, 0, p));
  }
  if (f[0] == "snappy") {
    if (old)
      return std::unique_ptr<hipcomp::hipcompManagerBase>(new hipcomp::SnappyManager(chunk));
    return std::unique_ptr<hipcomp::hipcompManagerBase>(new hipcomp::SnappyManager(chunk, 0, 0, p));
  }
  hipcompBatchedCascadedOpts_t o = hipcompBatchedCascadedDefaultOpts;
  o.chunk_size = chunk;
  o.type = (hipcompType_t)std::atoi(f.at(2).c_str());
  o.num_RLEs = std::atoi(f.at(3).c_str());
  o.num_deltas = std::atoi(f.at(4).c_str());
  o.use_bp = std::atoi(f.at(5).c_str());
  if (old)
    return std::unique_ptr<hipcomp::hipcompManagerBase>(new hipcomp::CascadedManager(o));
  return std::unique_ptr<hipcomp::hipcompManagerBase>(new hipcomp::CascadedManager(o, 0, 0, p));
}

static uint8_t* own_scratch(hipcomp::hipcompManagerBase& m, size_t* bytes)
{
  uint8_t* s = nullptr;
  *bytes = m.get_required_scratch_buffer_size();
  HIP(hipMalloc((void**)&s, *bytes));
  m.set_scratch_buffer(s);
  return s;
}

static int compress(const std::string& codec, const std::string& policy, const char* in, const char* out, bool scratch)
{
  const std::vector<uint8_t> data = read_file(in);
  std::unique_ptr<hipcomp::hipcompManagerBase> m = make_manager(codec, policy);
  size_t scratch_bytes = m->get_required_scratch_buffer_size();
  uint8_t* s = scratch ? own_scratch(*m, &scratch_bytes) : nullptr;
  uint8_t *d_in = nullptr, *d_out = nullptr;
  HIP(hipMalloc((void**)&d_in, data.size() + 16));
  if (!data.empty())
    HIP(hipMemcpy(d_in, data.data(), data.size(), hipMemcpyHostToDevice));
  hipcomp::CompressionConfig cfg = m->configure_compression(data.size());
  HIP(hipMalloc((void**)&d_out, cfg.max_compressed_buffer_size));
  m->compress(d_in, d_out, cfg);
  HIP(hipDeviceSynchronize());
  const size_t bytes = m->get_compressed_output_size(d_out);
  std::vector<uint8_t> c(bytes);
  HIP(hipMemcpy(c.data(), d_out, bytes, hipMemcpyDeviceToHost));
  write_file(out, c.data(), bytes);
  std::printf("status %d scratch %zu\n", (int)*cfg.get_status(), scratch_bytes);
  m.reset();
  HIP(hipFree(d_in));
  HIP(hipFree(d_out));
  if (s)
    HIP(hipFree(s));
  return 0;
}

static int decompress(const std::string& policy, const char* in, const char* out, bool scratch)
{
  const std::vector<uint8_t> c = read_file(in);
  uint8_t *d_in = nullptr, *d_out = nullptr;
  // (create_manager copies the common header and the largest format header: 88 bytes, more than a container of
  // an empty LZ4 or Snappy buffer holds)
  HIP(hipMalloc((void**)&d_in, c.size() + 128));
  HIP(hipMemcpy(d_in, c.data(), c.size(), hipMemcpyHostToDevice));
  std::shared_ptr<hipcomp::hipcompManagerBase> m =
      policy == "old" ? hipcomp::create_manager(d_in)
                      : hipcomp::create_manager(d_in, 0, 0, (hipcomp::ChecksumPolicy)std::atoi(policy.c_str()));
  size_t scratch_bytes = 0;
  uint8_t* s = scratch ? own_scratch(*m, &scratch_bytes) : nullptr;
  hipcomp::DecompressionConfig cfg = m->configure_decompression(d_in);
  HIP(hipMalloc((void**)&d_out, cfg.decomp_data_size + 16));
  m->decompress(d_out, d_in, cfg);
  HIP(hipDeviceSynchronize());
  std::vector<uint8_t> d(cfg.decomp_data_size);
  if (!d.empty())
    HIP(hipMemcpy(d.data(), d_out, d.size(), hipMemcpyDeviceToHost));
  write_file(out, d.data(), d.size());
  std::printf("status %d\n", (int)*cfg.get_status());
  m.reset();
  HIP(hipFree(d_in));
  HIP(hipFree(d_out));
  if (s)
    HIP(hipFree(s));
  return 0;
}

static int timing(size_t chunks, int reps)
{
  const size_t chunk = 65536, n = chunks * chunk;
  uint8_t *d_in = nullptr, *d_out = nullptr, *d_back = nullptr;
  HIP(hipMalloc((void**)&d_in, n));
  HIP(hipMalloc((void**)&d_back, n));
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
  for (hipcomp::ChecksumPolicy p : {hipcomp::NoComputeNoVerify, hipcomp::ComputeAndVerify}) {
    hipcomp::LZ4Manager m(chunk, HIPCOMP_TYPE_CHAR, 0, 0, p);
    hipcomp::CompressionConfig cfg = m.configure_compression(n);
    if (!d_out)
      HIP(hipMalloc((void**)&d_out, cfg.max_compressed_buffer_size));
    hipcomp::DecompressionConfig dcfg = m.configure_decompression(cfg);
    float cms = 0, dms = 0;
    for (int r = 0; r < reps + 1; ++r) { // (the first of each: warm-up)
      float ms = 0;
      HIP(hipEventRecord(a, 0));
      m.compress(d_in, d_out, cfg);
      HIP(hipEventRecord(b, 0));
      HIP(hipEventSynchronize(b));
      HIP(hipEventElapsedTime(&ms, a, b));
      if (r)
        cms += ms;
      HIP(hipEventRecord(a, 0));
      m.decompress(d_back, d_out, dcfg);
      HIP(hipEventRecord(b, 0));
      HIP(hipEventSynchronize(b));
      HIP(hipEventElapsedTime(&ms, a, b));
      if (r)
        dms += ms;
    }
    std::printf("policy %d compress_ms %.4f decompress_ms %.4f status %d %d\n", (int)p, cms / reps, dms / reps,
                (int)*cfg.get_status(), (int)*dcfg.get_status());
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
    if (cmd == "compress" && argc >= 6)
      return compress(argv[2], argv[3], argv[4], argv[5], argc > 6 && std::string(argv[6]) == "scratch");
    if (cmd == "decompress" && argc >= 5)
      return decompress(argv[2], argv[3], argv[4], argc > 5 && std::string(argv[5]) == "scratch");
    if (cmd == "timing" && argc == 4)
      return timing(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 4;
  }
  std::fprintf(stderr, "usage: see the head of hlif_checksum_driver.cpp\n");
  return 2;
}
