// The arithmetic of a read of a batch of LZ4 frames (hipcomp-core_amd/csrc/lz4_frames_plan.hpp) printed for
// tests/test_lz4_frames_plan_cpu.py, which compiles this with g++ -fsanitize=address,undefined and no HIP.
//   lz4_frames_plan_driver layout ITEMS P ROOM MOST
//       "items_bytes A totals_at B ticket_at C lists_at D item_column_at E scratch_bytes F min_scratch_bytes G pass_entries H"
//   lz4_frames_plan_driver passes P COUNT...
//       the block counts of the items in order; first a line "total T passes N", then per pass "pass K count C" and
//       per item with entries in it "pass K item I at A count C"
//   lz4_frames_plan_driver prefix PREFIX ITEM_BYTES WORD CAPACITY     (WORD: a signed 64-bit number)
//       "kind K payload_at A expected E size S"  (E: -1 where there is none)
#include "lz4_frames_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace hcamd::lz4fb;

int main(int argc, char** argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "layout" && argc == 6) {
    const uint64_t items = std::strtoull(argv[2], nullptr, 0), P = std::strtoull(argv[3], nullptr, 0),
                   room = std::strtoull(argv[4], nullptr, 0), most = std::strtoull(argv[5], nullptr, 0);
    std::printf("items_bytes %llu totals_at %llu ticket_at %llu lists_at %llu item_column_at %llu scratch_bytes %llu "
                "min_scratch_bytes %llu pass_entries %llu\n",
                (unsigned long long)items_bytes(items), (unsigned long long)totals_at(items), (unsigned long long)ticket_at(items),
                (unsigned long long)lists_at(items), (unsigned long long)item_column_at(items, P),
                (unsigned long long)scratch_bytes(items, P), (unsigned long long)min_scratch_bytes(items),
                (unsigned long long)pass_entries(room, items, most));
    return 0;
  }
  if (cmd == "passes" && argc >= 3) {
    const uint64_t P = std::strtoull(argv[2], nullptr, 0);
    std::vector<uint64_t> counts, first;
    uint64_t total = 0;
    for (int a = 3; a < argc; ++a) {
      counts.push_back(std::strtoull(argv[a], nullptr, 0));
      first.push_back(total);
      total += counts.back();
    }
    const uint64_t passes = passes_of(total, P);
    std::printf("total %llu passes %llu\n", (unsigned long long)total, (unsigned long long)passes);
    for (uint64_t k = 0; k < passes; ++k) {
      std::printf("pass %llu count %llu\n", (unsigned long long)k, (unsigned long long)pass_count(total, P, k));
      for (size_t i = 0; i < counts.size(); ++i) {
        const Slice s = item_slice(first[i], counts[i], P, k);
        if (s.count)
          std::printf("pass %llu item %zu at %llu count %llu\n", (unsigned long long)k, i, (unsigned long long)s.at,
                      (unsigned long long)s.count);
      }
    }
    return 0;
  }
  if (cmd == "prefix" && argc == 6) {
    const uint32_t prefix = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint64_t bytes = std::strtoull(argv[3], nullptr, 0), word = (uint64_t)std::strtoll(argv[4], nullptr, 0),
                   capacity = std::strtoull(argv[5], nullptr, 0);
    const PrefixPlan p = prefix_plan(prefix, bytes, word, capacity);
    std::printf("kind %u payload_at %llu expected %lld size %llu\n", p.kind, (unsigned long long)p.payload_at,
                p.expected == kNoExpectedSize ? -1ll : (long long)p.expected, (unsigned long long)prefix_size(bytes, word));
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of lz4_frames_plan_driver.cpp\n");
  return 2;
}
