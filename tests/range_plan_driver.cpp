// Prints the plan of a ranged read (hipcomp-core_amd/csrc/range_plan.hpp) for tests/test_range_plan_cpu.py.
// Standard headers only, no HIP.  Reads cases from standard input, one per line:
//   decomp_bytes chunk_bytes first_byte num_bytes slab edge_slots align out_mod elem
// and prints for each either "refused" or
//   plan first_chunk F chunks N all_edge A per_pass P passes K
//   chunk C pass K edge E slot S src A dst B bytes N cap M      (every chunk; of more than 64 the first and last 8)
// and then "end".
#include "range_plan.hpp"

#include <cinttypes>
#include <cstdio>

using namespace hcamd::range;

// (the plan is constexpr: the kernels and the host evaluate the same functions)
constexpr bool kPlanned = [] {
  Plan p;
  return range_plan(p, 33, 7, 5, 20, 4, 2, 1, 0, 1) && p.first_chunk == 0 && p.chunks == 4 && !p.all_edge
         && range_span(p, 0, 0).edge && !range_span(p, 1, 0).edge && range_span(p, 3, 0).slot == 1;
}();
static_assert(kPlanned, "range_plan");

int main()
{
  unsigned long long d, c, f, n, slab, slots, align, mod, elem;
  while (std::scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu", &d, &c, &f, &n, &slab, &slots, &align, &mod, &elem) == 9) {
    Plan p;
    if (!range_plan(p, d, c, f, n, (uint32_t)slab, (uint32_t)slots, (uint32_t)align, (uint32_t)mod, (uint32_t)elem)) {
      std::printf("refused\nend\n");
      continue;
    }
    std::printf("plan first_chunk %" PRIu64 " chunks %" PRIu64 " all_edge %u per_pass %u passes %" PRIu64 "\n", p.first_chunk,
                p.chunks, p.all_edge, p.per_pass, p.passes);
    for (uint64_t k = 0; k < p.passes; ++k) {
      const uint64_t first = range_pass_first(p, k);
      const uint32_t count = range_pass_count(p, k);
      for (uint32_t i = 0; i < count; ++i) {
        const uint64_t chunk = first + i, at = chunk - p.first_chunk;
        if (p.chunks > 64 && at >= 8 && at < p.chunks - 8)
          continue;
        const Span s = range_span(p, chunk, first);
        std::printf("chunk %" PRIu64 " pass %" PRIu64 " edge %d slot %u src %" PRIu64 " dst %" PRIu64 " bytes %" PRIu64
                    " cap %" PRIu64 "\n",
                    chunk, k, s.edge ? 1 : 0, s.slot, s.src_at, s.dst_at, s.bytes, s.cap);
      }
      if (p.chunks > 64 && k >= 2 && k + 3 < p.passes)
        k = p.passes - 3; // (a plan of very many passes: its first and last ones)
    }
    std::printf("end\n");
  }
  return 0;
}
