// Reads of many ranges in one call (hipcomp/hipcompManager.hpp, decompress_ranges) driven on files, for
// tests/test_hlif_ranges_gpu.py and scripts/quick_ranges.py.  Written against include/ and linked to libhipcomp.so.
//   hlif_ranges_driver compress CODEC POLICY IN OUT
//       CODEC: lz4:CHUNK:TYPE | snappy:CHUNK | cascaded:CHUNK:TYPE:RLES:DELTAS:BP
//       POLICY: 0..4 (the ChecksumPolicy) or "old" (the constructor without a policy); prints "status S"
//   hlif_ranges_driver ranges CODEC POLICY CASE [-- CASE ...]
//       CASE: CONTAINER RANGES OUT [out_misalign] [scratch] [nooffs] [cmp] [out_bytes=N] [poke=AT:XOR ...]
//       RANGES: a file of (first, num) pairs of little-endian u64.  Per case a manager of CODEC with the policy;
//       configure_decompression(container), then every poke (byte AT of the container on the device ^= XOR), the
//       ranges copied to the device, then decompress_ranges into a buffer that lies out_misalign bytes off a 256-byte
//       boundary between 64 guard bytes on each side, out_bytes = the sum of the lengths of the ranges that lie
//       inside the buffer (or N), and an offsets array of ranges + 1 words between 8 guard words on each side, all of
//       it filled with 0xA5 (nooffs: a null pointer).  OUT gets out[0, that sum), OUT.offs the offsets array.
//       scratch: a caller-owned scratch buffer of exactly get_required_scratch_buffer_size() bytes with 256 guard
//       bytes behind it.  cmp: also decompress_range every range with the same manager and compare.
//       prints per case "status S guards G offs_guards O scratch_guard H ranges R touched T passes P total B
//       pass_chunks C [same_as_range E]" (G, O, H: 1 = intact)
//   hlif_ranges_driver pass_chunks CODEC POLICY [scratch]      prints "pass_chunks C"
//   hlif_ranges_driver timing CHUNKS REPS [FILE]
//       the LZ4 manager, CHUNKS x 64 KiB of uniform random bytes (or of FILE's bytes, repeated): one decompress_ranges
//       of R ranges of 256 bytes at seeded random places against R calls of decompress_range, R = 1, 16, 1024, 16384,
//       and against a decompress of everything; then ranges of one chunk each that cover every chunk against
//       decompress.  NoComputeNoVerify and ComputeAndVerify; host clock around call(s) plus stream synchronisation,
//       the calls alternate inside every repetition, 2 warm-up repetitions, median of REPS, milliseconds
#include "hipcomp/hipcompManagerFactory.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
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

static void write_file(const std::string& path, const uint8_t* p, size_t n)
{
  FILE* f = std::fopen(path.c_str(), "wb");
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

// one of the three managers: the ranged reads are members of each, not of their base
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
  void decompress_ranges(uint8_t* out, size_t out_bytes, const uint8_t* comp, const hipcomp::DecompressionConfig& cfg,
                         const size_t* first, const size_t* num, size_t ranges, size_t* offs)
  {
    if (lz4)
      lz4->decompress_ranges(out, out_bytes, comp, cfg, first, num, ranges, offs);
    else if (snappy)
      snappy->decompress_ranges(out, out_bytes, comp, cfg, first, num, ranges, offs);
    else
      cascaded->decompress_ranges(out, out_bytes, comp, cfg, first, num, ranges, offs);
  }
  size_t pass_chunks() const
  {
    return lz4 ? lz4->get_ranges_pass_chunks() : snappy ? snappy->get_ranges_pass_chunks() : cascaded->get_ranges_pass_chunks();
  }
  hipcomp::RangesStats stats() const
  {
    return lz4 ? lz4->get_ranges_stats() : snappy ? snappy->get_ranges_stats() : cascaded->get_ranges_stats();
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

constexpr size_t kGuard = 64, kOffsGuard = 8, kScratchGuard = 256;
constexpr uint8_t kGuardByte = 0xA5, kScratchGuardByte = 0x5C;

static int ranges_case(const std::string& codec, const std::string& policy, const std::vector<std::string>& a)
{
  if (a.size() < 3)
    return 2;
  const std::vector<uint8_t> c = read_file(a[0].c_str());
  const std::vector<uint8_t> rf = read_file(a[1].c_str());
  const std::string out_path = a[2];
  size_t misalign = 0, out_bytes = 0;
  bool scratch = false, nooffs = false, cmp = false, out_bytes_given = false;
  std::vector<std::pair<size_t, unsigned>> pokes;
  for (size_t i = 3; i < a.size(); ++i) {
    if (a[i] == "scratch")
      scratch = true;
    else if (a[i] == "nooffs")
      nooffs = true;
    else if (a[i] == "cmp")
      cmp = true;
    else if (a[i].rfind("out_bytes=", 0) == 0) {
      out_bytes = std::strtoull(a[i].c_str() + 10, nullptr, 0);
      out_bytes_given = true;
    } else if (a[i].rfind("poke=", 0) == 0) {
      const std::vector<std::string> f = split(a[i].substr(5));
      pokes.emplace_back(std::strtoull(f.at(0).c_str(), nullptr, 0), (unsigned)std::strtoul(f.at(1).c_str(), nullptr, 0));
    } else
      misalign = std::strtoull(a[i].c_str(), nullptr, 0);
  }
  const size_t R = rf.size() / 16;
  std::vector<size_t> first(R), num(R);
  for (size_t r = 0; r < R; ++r) {
    std::memcpy(&first[r], &rf[16 * r], 8);
    std::memcpy(&num[r], &rf[16 * r + 8], 8);
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
  // (a range the call must refuse gets no room)
  size_t room = 0;
  for (size_t r = 0; r < R; ++r)
    if (first[r] <= cfg.decomp_data_size && num[r] <= cfg.decomp_data_size - first[r])
      room += num[r];
  if (!out_bytes_given)
    out_bytes = room;
  const size_t total = 256 + kGuard + room + kGuard;
  uint8_t* d_buf = nullptr;
  HIP(hipMalloc((void**)&d_buf, total));
  HIP(hipMemset(d_buf, kGuardByte, total));
  uint8_t* const d_out = d_buf + 256 + misalign; // misalign bytes behind a 256-byte boundary
  size_t *d_first = nullptr, *d_num = nullptr, *d_offs_buf = nullptr;
  HIP(hipMalloc((void**)&d_first, 8 * R + 8));
  HIP(hipMalloc((void**)&d_num, 8 * R + 8));
  const size_t offs_words = kOffsGuard + R + 1 + kOffsGuard;
  HIP(hipMalloc((void**)&d_offs_buf, 8 * offs_words));
  HIP(hipMemset(d_offs_buf, kGuardByte, 8 * offs_words));
  if (R) {
    HIP(hipMemcpy(d_first, first.data(), 8 * R, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_num, num.data(), 8 * R, hipMemcpyHostToDevice));
  }
  m.decompress_ranges(d_out, out_bytes, d_in, cfg, d_first, d_num, R, nooffs ? nullptr : d_offs_buf + kOffsGuard);
  HIP(hipDeviceSynchronize());
  const int status = (int)*cfg.get_status();
  const hipcomp::RangesStats st = m.stats();
  std::vector<uint8_t> h(total);
  HIP(hipMemcpy(h.data(), d_buf, total, hipMemcpyDeviceToHost));
  const size_t at = (size_t)(d_out - d_buf);
  bool guards = true;
  for (size_t i = 0; i < total; ++i)
    if ((i < at || i >= at + room) && h[i] != kGuardByte)
      guards = false;
  write_file(out_path, h.data() + at, room);
  std::vector<uint8_t> ho(8 * offs_words);
  HIP(hipMemcpy(ho.data(), d_offs_buf, ho.size(), hipMemcpyDeviceToHost));
  bool offs_guards = true;
  for (size_t i = 0; i < ho.size(); ++i)
    if ((i < 8 * kOffsGuard || i >= 8 * (kOffsGuard + R + 1) || nooffs) && ho[i] != kGuardByte)
      offs_guards = false;
  write_file(out_path + ".offs", ho.data() + 8 * kOffsGuard, 8 * (R + 1));
  bool scratch_guard = true;
  if (s) {
    std::vector<uint8_t> g(kScratchGuard);
    HIP(hipMemcpy(g.data(), s + scratch_bytes, kScratchGuard, hipMemcpyDeviceToHost));
    for (uint8_t b : g)
      scratch_guard = scratch_guard && b == kScratchGuardByte;
  }
  std::printf("status %d guards %d offs_guards %d scratch_guard %d ranges %zu touched %zu passes %zu total %zu pass_chunks %zu",
              status, guards ? 1 : 0, offs_guards ? 1 : 0, scratch_guard ? 1 : 0, st.ranges, st.touched_chunks, st.passes,
              st.total_bytes, m.pass_chunks());
  if (cmp) {
    bool same = status == 0;
    size_t most = 1;
    for (size_t r = 0; r < R; ++r)
      most = std::max(most, num[r]);
    uint8_t* d_one = nullptr;
    HIP(hipMalloc((void**)&d_one, most + 16));
    std::vector<uint8_t> one(most);
    size_t off = 0;
    for (size_t r = 0; r < R && same; ++r) {
      hipcomp::DecompressionConfig cfg2 = m.base().configure_decompression(d_in);
      m.decompress_range(d_one + 1, d_in, cfg2, first[r], num[r]);
      HIP(hipDeviceSynchronize());
      if (num[r])
        HIP(hipMemcpy(one.data(), d_one + 1, num[r], hipMemcpyDeviceToHost));
      same = *cfg2.get_status() == hipcompSuccess && std::memcmp(one.data(), h.data() + at + off, num[r]) == 0;
      off += num[r];
    }
    std::printf(" same_as_range %d", same ? 1 : 0);
    HIP(hipFree(d_one));
  }
  std::printf("\n");
  m = Manager();
  HIP(hipFree(d_in));
  HIP(hipFree(d_buf));
  HIP(hipFree(d_first));
  HIP(hipFree(d_num));
  HIP(hipFree(d_offs_buf));
  if (s)
    HIP(hipFree(s));
  return 0;
}

static int pass_chunks(const std::string& codec, const std::string& policy, bool scratch)
{
  Manager m = make_manager(codec, policy);
  uint8_t* s = nullptr;
  if (scratch) {
    HIP(hipMalloc((void**)&s, m.base().get_required_scratch_buffer_size()));
    m.base().set_scratch_buffer(s);
  }
  std::printf("pass_chunks %zu\n", m.pass_chunks());
  m = Manager();
  if (s)
    HIP(hipFree(s));
  return 0;
}

static double now_ms()
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int timing(size_t chunks, int reps, const char* file)
{
  const size_t chunk = 65536, n = chunks * chunk;
  uint8_t *d_in = nullptr, *d_out = nullptr, *d_back = nullptr;
  HIP(hipMalloc((void**)&d_in, n));
  HIP(hipMalloc((void**)&d_back, n + 64));
  {
    std::vector<uint8_t> h(n);
    if (file) {
      const std::vector<uint8_t> piece = read_file(file);
      if (piece.empty())
        return 2;
      for (size_t i = 0; i < n; i += piece.size())
        std::memcpy(&h[i], piece.data(), std::min(piece.size(), n - i));
    } else {
      uint64_t x = 0x9E3779B97F4A7C15ull;
      for (size_t i = 0; i < n; i += 8) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        std::memcpy(&h[i], &x, 8);
      }
    }
    HIP(hipMemcpy(d_in, h.data(), n, hipMemcpyHostToDevice));
  }
  const size_t row = 256, counts[] = {1, 16, 1024, 16384};
  const size_t most = std::max<size_t>(16384, chunks);
  size_t *d_first = nullptr, *d_num = nullptr;
  HIP(hipMalloc((void**)&d_first, 8 * most));
  HIP(hipMalloc((void**)&d_num, 8 * most));
  for (hipcomp::ChecksumPolicy p : {hipcomp::NoComputeNoVerify, hipcomp::ComputeAndVerify}) {
    hipcomp::LZ4Manager m(chunk, HIPCOMP_TYPE_CHAR, 0, 0, p);
    hipcomp::CompressionConfig cfg = m.configure_compression(n);
    if (!d_out)
      HIP(hipMalloc((void**)&d_out, cfg.max_compressed_buffer_size));
    m.compress(d_in, d_out, cfg);
    HIP(hipDeviceSynchronize());
    hipcomp::DecompressionConfig dcfg = m.configure_decompression(cfg);
    int worst = 0;
    for (int k = 0; k < 5; ++k) {
      // rows 0..3: R ranges of 256 bytes at seeded random places; row 4: a range per chunk, every chunk
      const bool cover = k == 4;
      const size_t R = cover ? chunks : counts[k];
      std::vector<size_t> first(R), num(R);
      uint64_t x = 0xD1B54A32D192ED03ull + k;
      for (size_t r = 0; r < R; ++r) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        first[r] = cover ? r * chunk : (size_t)(x % (n - row));
        num[r] = cover ? chunk : row;
      }
      HIP(hipMemcpy(d_first, first.data(), 8 * R, hipMemcpyHostToDevice));
      HIP(hipMemcpy(d_num, num.data(), 8 * R, hipMemcpyHostToDevice));
      std::vector<double> one, loop, all;
      for (int rep = 0; rep < reps + 2; ++rep) {
        double t0 = now_ms();
        m.decompress_ranges(d_back + 1, n, d_out, dcfg, d_first, d_num, R, nullptr);
        HIP(hipStreamSynchronize(0));
        double t1 = now_ms();
        worst = std::max(worst, (int)*dcfg.get_status());
        if (rep >= 2)
          one.push_back(t1 - t0);
        if (!cover) {
          t0 = now_ms();
          for (size_t r = 0; r < R; ++r)
            m.decompress_range(d_back + 1 + r * row, d_out, dcfg, first[r], row);
          HIP(hipStreamSynchronize(0));
          t1 = now_ms();
          worst = std::max(worst, (int)*dcfg.get_status());
          if (rep >= 2)
            loop.push_back(t1 - t0);
        }
        t0 = now_ms();
        m.decompress(d_back, d_out, dcfg);
        HIP(hipStreamSynchronize(0));
        t1 = now_ms();
        worst = std::max(worst, (int)*dcfg.get_status());
        if (rep >= 2)
          all.push_back(t1 - t0);
      }
      const auto median = [](std::vector<double>& v) {
        std::sort(v.begin(), v.end());
        return v.empty() ? 0.0 : v[v.size() / 2];
      };
      const hipcomp::RangesStats st = m.get_ranges_stats();
      std::printf("policy %d %-6s ranges %6zu bytes_each %6zu touched %6zu passes %zu one_call_ms %.4f loop_of_calls_ms %.4f "
                  "decompress_all_ms %.4f\n",
                  (int)p, cover ? "cover" : "rows", R, num[0], st.touched_chunks, st.passes, median(one), median(loop), median(all));
    }
    std::printf("policy %d worst_status %d\n", (int)p, worst);
  }
  HIP(hipFree(d_in));
  HIP(hipFree(d_out));
  HIP(hipFree(d_back));
  HIP(hipFree(d_first));
  HIP(hipFree(d_num));
  return 0;
}

int main(int argc, char** argv)
{
  try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "compress" && argc == 6)
      return compress(argv[2], argv[3], argv[4], argv[5]);
    if (cmd == "ranges" && argc >= 7) {
      std::vector<std::string> group;
      for (int i = 4; i <= argc; ++i) {
        if (i == argc || std::string(argv[i]) == "--") {
          const int rc = ranges_case(argv[2], argv[3], group);
          if (rc)
            return rc;
          group.clear();
        } else
          group.push_back(argv[i]);
      }
      return 0;
    }
    if (cmd == "pass_chunks" && argc >= 4)
      return pass_chunks(argv[2], argv[3], argc > 4 && std::string(argv[4]) == "scratch");
    if (cmd == "timing" && (argc == 4 || argc == 5))
      return timing(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]), argc == 5 ? argv[4] : nullptr);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 4;
  }
  std::fprintf(stderr, "usage: see the head of hlif_ranges_driver.cpp\n");
  return 2;
}
