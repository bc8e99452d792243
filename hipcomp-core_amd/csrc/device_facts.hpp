// device_facts.hpp -- what the launchers of every codec know about the device they launch on.  Facts
// that have to be asked for are asked once per device (the calling thread's current one: a process may
// drive several GPUs, one thread each, as the reference's callers do) and kept (device_facts.cpp).
// Standard headers only: the LZ4 launch plan (lz4_plan.cpp) is compiled and tested without HIP.
#pragma once

#include <cstdint>

namespace hcamd {

// LDS of one CU, handed out to workgroups in granules (scripts/probes/lds_occupancy.hip)
constexpr uint32_t kLdsPerCu = 160u * 1024u;
constexpr uint32_t kLdsGranule = 1280u;

// workgroups with `lds_bytes` of LDS each that the LDS of one CU holds
constexpr uint32_t groups_by_lds(uint32_t lds_bytes)
{
  return kLdsPerCu / (((lds_bytes ? lds_bytes : 1u) + kLdsGranule - 1u) / kLdsGranule * kLdsGranule);
}

// the calling thread's current device; -1: none, or one beyond the per-device state kept here
int current_device();

// compute units of the current device (256 where that cannot be found out)
int num_cus_of_current_device();

// workgroups of `kernel` with `block` threads and `lds_bytes` of dynamic LDS that one CU of the current
// device holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor, asked once per device and kernel
// shape); 0: could not be found out
int resident_per_cu(const void* kernel, int block, uint32_t lds_bytes);

// `raise` (which returns a hipError_t) is called on the first call per device; returns what it returned
// then (a launcher's once-per-device setup: lz4_kernels.hip raises its kernels' dynamic-LDS limit)
int raise_dynamic_lds_once(int (*raise)());

} // namespace hcamd
