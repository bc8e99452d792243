// Prints the arithmetic of a read of many ranges (hipcomp-core_amd/csrc/gather_plan.hpp) for
// tests/test_gather_plan_cpu.py.  Standard headers only, no HIP.  Reads cases from standard input, one per line:
//   range decomp_bytes chunk_bytes first num elem
//       "refused", or "range c0 A c1 B" (num > 0; "range empty" else) and for every chunk of [c0, c1] (of more than
//       64 the first and last 8) "piece chunk C src A bytes N dst B cap M"
//   rank rank_c0 c0 c1 S pass
//       "rank lo A hi B" (the chunks of [c0, c1] the pass decodes), and for each of them (up to 64)
//       "chunk C rank R pass P slot K"
//   pass touched S          "pass passes P" and "count K" for every pass (up to 64)
//   room room stride ranges num_chunks cap
//       "room tables T slots S back B" (B: room_of(S, stride, T))
//   sat a b                 "sat S refused_at_b R"  (sat_add(a, b), total_refused(a, b))
//   bits word bit           "bits N"
// and then "end" behind each.
#include "gather_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace hcamd::gather;

// (the arithmetic is constexpr: the kernels and the host evaluate the same functions)
static_assert(range_valid(100, 99, 1, 1) && !range_valid(100, 99, 2, 1) && !range_valid(100, 1, ~uint64_t(0), 1), "range_valid");
static_assert(range_chunks(7, 5, 20).c0 == 0 && range_chunks(7, 5, 20).c1 == 3, "range_chunks");
static_assert(range_piece(33, 7, 5, 20, 0).bytes == 2 && range_piece(33, 7, 5, 20, 3).dst_at == 16, "range_piece");
static_assert(pass_of(7, 3) == 2 && slot_of(7, 3) == 1 && passes_of(7, 3) == 3 && pass_count(7, 3, 2) == 1, "passes");
static_assert(sat_add(~uint64_t(0) - 1, 5) == ~uint64_t(0) && sat_add(2, 3) == 5, "sat_add");

int main()
{
  char what[16];
  unsigned long long v[6];
  while (std::scanf("%15s", what) == 1) {
    if (!std::strcmp(what, "range")) {
      if (std::scanf("%llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5)
        return 1;
      const uint64_t d = v[0], c = v[1], f = v[2], n = v[3];
      if (!range_valid(d, f, n, (uint32_t)v[4]))
        std::printf("refused\n");
      else if (n == 0)
        std::printf("range empty\n");
      else {
        const Interval iv = range_chunks(c, f, n);
        std::printf("range c0 %" PRIu64 " c1 %" PRIu64 "\n", iv.c0, iv.c1);
        const uint64_t chunks = iv.c1 - iv.c0 + 1;
        for (uint64_t k = 0; k < chunks; ++k) {
          if (chunks > 64 && k == 8)
            k = chunks - 8;
          const Piece p = range_piece(d, c, f, n, iv.c0 + k);
          std::printf("piece chunk %" PRIu64 " src %" PRIu64 " bytes %" PRIu64 " dst %" PRIu64 " cap %" PRIu64 "\n", iv.c0 + k,
                      p.src_at, p.bytes, p.dst_at, chunk_cap(d, c, iv.c0 + k));
        }
      }
    } else if (!std::strcmp(what, "rank")) {
      if (std::scanf("%llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5)
        return 1;
      const InPass in = range_in_pass(v[0], v[1], v[2], v[3], v[4]);
      std::printf("rank lo %" PRIu64 " hi %" PRIu64 "\n", in.lo, in.hi);
      for (uint64_t c = in.lo, k = 0; c < in.hi && k < 64; ++c, ++k) {
        const uint64_t r = rank_in_range(v[0], v[1], c);
        std::printf("chunk %" PRIu64 " rank %" PRIu64 " pass %" PRIu64 " slot %" PRIu64 "\n", c, r, pass_of(r, v[3]), slot_of(r, v[3]));
      }
    } else if (!std::strcmp(what, "pass")) {
      if (std::scanf("%llu %llu", &v[0], &v[1]) != 2)
        return 1;
      const uint64_t passes = passes_of(v[0], v[1]);
      std::printf("pass passes %" PRIu64 "\n", passes);
      for (uint64_t p = 0; p < passes && p < 64; ++p)
        std::printf("count %" PRIu64 "\n", pass_count(v[0], v[1], p));
    } else if (!std::strcmp(what, "room")) {
      if (std::scanf("%llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5)
        return 1;
      const uint64_t t = table_bytes(v[2], v[3]), s = slots_of(v[0], v[1], t, v[4]);
      std::printf("room tables %" PRIu64 " slots %" PRIu64 " back %" PRIu64 "\n", t, s, room_of(s, v[1], t));
    } else if (!std::strcmp(what, "sat")) {
      if (std::scanf("%llu %llu", &v[0], &v[1]) != 2)
        return 1;
      std::printf("sat %" PRIu64 " refused_at_b %d\n", sat_add(v[0], v[1]), total_refused(v[0], v[1]) ? 1 : 0);
    } else if (!std::strcmp(what, "bits")) {
      if (std::scanf("%llu %llu", &v[0], &v[1]) != 2)
        return 1;
      std::printf("bits %u\n", bits_below((uint32_t)v[0], (uint32_t)v[1]));
    } else
      return 1;
    std::printf("end\n");
  }
  return 0;
}
