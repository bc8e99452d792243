// device_facts.cpp -- the per-device state behind device_facts.hpp.  Every step is idempotent, so a race
// between two first callers on one device is harmless; after the first call per device (and kernel
// shape) nothing is allocated and nothing is asked of the runtime but the current device.
#include "device_facts.hpp"

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <mutex>

namespace hcamd {

namespace {

constexpr int kMaxDevices = 64;
std::atomic<int> g_num_cus[kMaxDevices];
std::atomic<int> g_lds_raised[kMaxDevices]; // 0 = not yet, 1 = done, < 0 = -hipError

// Kernel shapes whose residency is known, per device: filled in order under the lock; an entry is
// there once its `per_cu` is (written last, read first).
constexpr int kShapesPerDevice = 16;
struct Resident
{
  const void* kernel;
  int block;
  uint32_t lds_bytes;
  std::atomic<int> per_cu;
};
Resident g_resident[kMaxDevices][kShapesPerDevice];
std::mutex g_resident_lock;

} // namespace

int current_device()
{
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices)
    return -1;
  return dev;
}

int num_cus_of_current_device()
{
  const int dev = current_device();
  if (dev < 0)
    return 256;
  int n = g_num_cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    g_num_cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int resident_per_cu(const void* kernel, int block, uint32_t lds_bytes)
{
  const int dev = current_device();
  Resident* known = dev >= 0 ? g_resident[dev] : nullptr;
  for (int i = 0; known && i < kShapesPerDevice; ++i) {
    const int n = known[i].per_cu.load(std::memory_order_acquire);
    if (n == 0)
      break;
    if (known[i].kernel == kernel && known[i].block == block && known[i].lds_bytes == lds_bytes)
      return n;
  }
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, lds_bytes) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return 0;
  }
  if (known) {
    std::lock_guard<std::mutex> hold(g_resident_lock);
    for (int i = 0; i < kShapesPerDevice; ++i) {
      Resident& r = known[i];
      if (r.per_cu.load(std::memory_order_relaxed) == 0) {
        r.kernel = kernel;
        r.block = block;
        r.lds_bytes = lds_bytes;
        r.per_cu.store(n, std::memory_order_release);
        break;
      }
      if (r.kernel == kernel && r.block == block && r.lds_bytes == lds_bytes)
        break;
    }
  }
  return n;
}

int raise_dynamic_lds_once(int (*raise)())
{
  const int dev = current_device();
  if (dev < 0)
    return hipErrorInvalidDevice;
  const int state = g_lds_raised[dev].load(std::memory_order_acquire);
  if (state == 1)
    return hipSuccess;
  if (state < 0)
    return -state;
  const int r = raise();
  g_lds_raised[dev].store(r == hipSuccess ? 1 : -r, std::memory_order_release);
  return r;
}

} // namespace hcamd
