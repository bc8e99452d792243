// lz4_plan_driver.cpp -- prints the LZ4 launch plan (hipcomp-core_amd/csrc/lz4_plan.cpp) for
// tests/test_lz4_plan_cpu.py, which compiles it with the planner alone (no HIP).
//   table    every call of the grid pinned in tests/lz4_plan_table.json, as the launches lz4_kernels.hip
//            makes of its plan: one record per kernel (name grid block lds, then the kernel's arguments that
//            the plan decides; a pointer into the temp buffer as h<header word>, l<class list>, r (retry
//            list), t (far tables), @<byte offset> (the decoder's ticket)), the layout first ("T")
//   plan ht batch elem_size max_chunk mode cus base_mod16 temp_bytes
//            one compress plan, field by field
//   layout   the temp layout's invariants for every base offset 0..15 (prints what is violated)
#include "lz4_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace hcamd;

namespace {

std::string out;
Lz4TempLayout lay;
size_t lay_batch;

void put(const std::string& s) { out += s; }
std::string num(size_t v) { return std::to_string(v); }
std::string off(size_t o) { return o == kAbsent ? "-" : num(o); }
void arg(size_t v) { put(" " + num(v)); }
void none() { put(" -"); }
void header_word(uint32_t w) { put(" h" + num(w)); }
void rec(const std::string& kernel, size_t grid, size_t block, size_t lds)
{
  if (!out.empty() && out.back() != ';')
    put(";");
  put(kernel + " " + num(grid) + " " + num(block) + " " + num(lds));
}

// lz4_kernels.hip, lz4_launch_compress, with the launches printed
int launch_compress(uint32_t ht, size_t batch, int es, size_t chunk, Lz4Mode mode, uint32_t cus, unsigned mod,
                    size_t bytes, bool placed)
{
  const Lz4CompressPlan p = lz4_plan_compress(ht, batch, es, chunk, mode, cus, mod, bytes, placed, Lz4Overrides());
  lay = p.temp;
  lay_batch = batch;
  put("T " + off(lay.header) + " " + off(lay.lists) + " " + off(lay.retry) + " " + off(lay.far_tables) + " "
      + num(lay.far_capacity));
  if (p.refused)
    return 1;
  const bool header = lay.header != kAbsent;
  // count / list: -1 none, 4 + class (its list), kHeaderRetryCount (the retry list)
  auto lds = [&](int count, uint32_t ticket_word, bool give) {
    const Lz4LdsLaunch& l = p.lds;
    rec((l.pair ? "pair" : "mix") + num(es), l.grid, l.waves * 64, l.lds_bytes);
    arg(ht);
    if (l.pair) {
      arg(l.pair_tags);
      arg(l.table_bytes);
    } else {
      arg(l.tagged);
      arg(l.stride_tagged);
      arg(l.stride_plain);
    }
    arg(batch);
    header ? header_word(ticket_word) : none();
    arg(l.per_ticket);
    if (count < 0) {
      none();
      none();
    } else {
      header_word(count);
      put(count == (int)kHeaderRetryCount ? " r" : " l" + num(count - 4));
    }
    put(" p");
    arg((give ? 1u : 0u) | (!l.pair && l.inpos ? 2u : 0u));
  };
  auto far = [&](uint32_t cls, bool routed) {
    const Lz4FarLaunch& g = p.far[cls];
    rec("far" + num(es) + "." + num(cls), g.groups, g.waves() * 64, g.lds_bytes);
    arg(ht);
    lay.far_tables != kAbsent ? put(" t") : none();
    arg(g.near);
    arg(g.slots);
    arg(g.span);
    arg(batch);
    header_word(cls);
    arg(g.per_ticket);
    arg(cls);
    if (routed) {
      put(" h4 l0 p");
      if (lay.retry != kAbsent)
        put(" h12 r");
      else
        put(" - -");
    } else
      put(" - - p - -");
  };
  if (!header) {
    lds(-1, kClassMix, false);
    return 0;
  }
  rec("zero", 1, kHeaderWords, 0);
  header_word(0);
  if (p.routed) {
    rec("route", p.route_grid, kRouteWaves * 64, 0);
    put(" - -");
    arg(batch);
    arg(p.route_per_group);
    put(" h0 l0");
    lds(4 + kClassMix, kClassMix, true);
    for (uint32_t cls = kClassDense; cls <= kClassWide; ++cls) {
      if (p.far[cls].groups == 0)
        return 1;
      far(cls, true);
    }
    if (lay.retry != kAbsent)
      lds(kHeaderRetryCount, kHeaderRetryTicket, false);
    return 0;
  }
  if (p.forced_far != kClassMix)
    far(p.forced_far, false);
  else
    lds(-1, kClassMix, false);
  return 0;
}

uint32_t calls = 0;

// lz4_kernels.hip, lz4_launch_decompress, with the launches printed
void launch_decompress(size_t batch, uint32_t cus, unsigned mod, size_t bytes, bool write_out)
{
  const Lz4DecompressPlan p = lz4_plan_decompress(batch, cus, mod, bytes);
  std::string ticket = "-";
  if (p.ticket_words) {
    ticket = "@" + num(p.ticket_offset(calls++));
    rec("zero", 1, 1, 0);
    put(" " + ticket);
  }
  rec(write_out ? "dec1" : "dec0", p.grid, 64 * kDecompWavesPerBlock, 0);
  put(" - - -");
  arg(batch);
  put(" - - - " + ticket);
}

uint32_t ht_of(size_t n)
{
  uint32_t ht = 1;
  while (ht < n)
    ht *= 2;
  return ht < 16384 ? ht : 16384;
}

void table()
{
  const size_t chunks[] = {512, 2048, 8192, 16384, 32768, 65536, 131072};
  const size_t batches[] = {1, 7, 100, 1000, 1024, 1536, 20000, 100000};
  for (int placed = 0; placed < 2; ++placed)
    for (int mode = 0; mode < 5; ++mode)
      for (uint32_t cus : {256u, 80u})
        for (int es : {1, 2, 4})
          for (size_t chunk : chunks)
            for (size_t batch : batches)
              for (int kind = 0; kind < 5; ++kind) // temp: none, 64 bytes, header + lists, contract, bytes used
                for (unsigned mod : {0u, 3u}) {
                  // forced shapes: 256 CUs, no buffer or the contract size; placement: the refusal
                  if (mode != 0 && (cus != 256 || (kind != 0 && kind != 3) || mod != 0 || placed))
                    continue;
                  if (placed && (cus != 256 || kind > 1 || mod != 0))
                    continue;
                  const uint32_t ht = ht_of(chunk);
                  const size_t bytes = kind == 0 ? 0 : kind == 1 ? 64 : kind == 2 ? 3 + 256 + 16 * batch
                                       : kind == 3 ? (size_t)ht * 2 * batch : lz4_compress_temp_bytes_used(ht, batch);
                  out.clear();
                  const int e = launch_compress(ht, batch, es, chunk, (Lz4Mode)mode, cus, mod, bytes, placed);
                  std::printf("C %u %d %d %zu %zu %d %u %d|%s%s;\n", cus, mode, es, chunk, batch, kind, mod, placed,
                              e ? "ERR;" : "", out.c_str());
                }
  for (uint32_t cus : {256u, 80u})
    for (size_t batch : batches)
      for (int kind = 0; kind < 3; ++kind) // temp: none, one word, the contract size
        for (unsigned mod : {0u, 3u})
          for (int pass = 0; pass < 2; ++pass) {
            out.clear();
            launch_decompress(batch, cus, mod, kind == 0 ? 0 : kind == 1 ? 4 : (24 * batch + 7) / 8 * 8, pass == 0);
            std::printf("D %u %zu %d %u %d|%s;\n", cus, batch, kind, mod, pass, out.c_str());
          }
  std::printf("U");
  for (size_t chunk : chunks)
    for (size_t batch : batches)
      std::printf(" %zu", lz4_compress_temp_bytes_used(ht_of(chunk), batch));
  std::printf("\n");
}

void plan(char** a)
{
  const uint32_t ht = (uint32_t)std::strtoul(a[0], nullptr, 10);
  const size_t batch = std::strtoull(a[1], nullptr, 10);
  const int es = std::atoi(a[2]);
  const size_t chunk = std::strtoull(a[3], nullptr, 10);
  const Lz4Mode mode = (Lz4Mode)std::atoi(a[4]);
  const uint32_t cus = (uint32_t)std::strtoul(a[5], nullptr, 10);
  const unsigned mod = (unsigned)std::atoi(a[6]);
  const size_t bytes = std::strtoull(a[7], nullptr, 10);
  const Lz4CompressPlan p = lz4_plan_compress(ht, batch, es, chunk, mode, cus, mod, bytes, false, Lz4Overrides());
  const Lz4LdsLaunch& l = p.lds;
  std::printf("routed %d route_grid %u route_per_group %u forced_far %u\n", p.routed, p.route_grid, p.route_per_group,
              p.forced_far);
  std::printf("lds pair %d grid %u waves %u lds_bytes %u per_ticket %u pair_tags %u tagged %u inpos %d\n", l.pair,
              l.grid, l.waves, l.lds_bytes, l.per_ticket, l.pair_tags, l.tagged, l.inpos);
  for (uint32_t cls = kClassDense; cls <= kClassWide; ++cls) {
    const Lz4FarLaunch& g = p.far[cls];
    std::printf("far%u groups %u near %u far %u slots %u lds_bytes %u span %u per_cu %u\n", cls, g.groups, g.near,
                g.far, g.slots, g.lds_bytes, g.span, g.groups / cus);
  }
}

void layout()
{
  for (uint32_t ht = 1; ht <= 16384; ht *= 2)
    for (size_t batch : {1, 7, 100, 1000, 8191, 8192, 8193, 20000, 100000})
      for (unsigned mod = 0; mod < 16; ++mod) {
        const size_t bytes = lz4_compress_temp_bytes_used(ht, batch);
        const Lz4TempLayout t = lz4_temp_layout(ht, batch, mod, bytes);
        const size_t table = (ht < 8 ? 8 : ht) * sizeof(uint16_t), want = batch < 8192 ? batch : 8192;
        auto fail = [&](const char* what) { std::printf("ht %u batch %zu base %u: %s\n", ht, batch, mod, what); };
        if (t.header == kAbsent || t.lists == kAbsent || t.retry == kAbsent || t.far_tables == kAbsent)
          fail("a part is missing");
        else if (t.far_capacity < want)
          fail("fewer tables than min(batch, 8192)");
        else if ((mod + t.header) % 4 || (mod + t.far_tables) % 16)
          fail("misaligned");
        else if (t.lists < t.header + kHeaderWords * 4 || t.retry < t.lists + kNumClasses * batch * 4
                 || t.far_tables < t.retry + batch * 4)
          fail("parts overlap");
        else if (t.far_tables + t.far_capacity * table > bytes)
          fail("past the end");
      }
}

} // namespace

int main(int argc, char** argv)
{
  if (argc >= 2 && std::strcmp(argv[1], "table") == 0)
    table();
  else if (argc >= 10 && std::strcmp(argv[1], "plan") == 0)
    plan(argv + 2);
  else if (argc >= 2 && std::strcmp(argv[1], "layout") == 0)
    layout();
  else
    return 2;
  return 0;
}
