// lz4_plan.cpp -- the launch plan of the LZ4 kernels (lz4_plan.hpp).  The geometries and why they are
// what they are: DESIGN.md §3.4; tests/test_lz4_plan_cpu.py pins them.
#include "lz4_plan.hpp"

namespace hcamd {

namespace {

uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }
size_t align(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }
uint32_t table_entries(uint32_t ht_size) { return ht_size < 8 ? 8u : ht_size; }

// The temp buffer's parts in their order: the alignment each one starts at and its bytes (the far tables:
// `tables` of them).  The layout and the bytes it uses at most are both read off this.
struct Part
{
  size_t align, bytes;
};
enum { kPartHeader, kPartLists, kPartRetry, kPartTables, kParts };
void temp_parts(uint32_t ht_size, size_t batch, size_t tables, Part part[kParts])
{
  part[kPartHeader] = {4, kHeaderWords * sizeof(uint32_t)};
  part[kPartLists] = {1, kNumClasses * batch * sizeof(uint32_t)};
  part[kPartRetry] = {1, batch * sizeof(uint32_t)};
  part[kPartTables] = {16, tables * table_entries(ht_size) * sizeof(uint16_t)};
}

// Workgroups of `waves` waves and `lds_bytes` of LDS one CU takes: as many as LDS holds, at most 8, at
// most 32 waves.
uint32_t groups_per_cu(uint32_t lds_bytes, uint32_t waves)
{
  uint32_t g = groups_by_lds(lds_bytes);
  if (g > 8)
    g = 8;
  if (g * waves > 32)
    g = 32 / waves;
  return g;
}

// The mix shape: per workgroup `tagged` waves whose chunk has a tag table behind its position table and
// `plain` waves without; as many persistent workgroups as fill every CU (late ones find the ticket counter
// exhausted and leave at once).
struct MixShape
{
  uint32_t tagged, plain, stride_tagged, stride_plain, lds_bytes, groups;
  uint32_t waves() const { return tagged + plain; }
};

void set_groups(MixShape& sh, size_t batch, uint32_t cus)
{
  const uint32_t w = sh.waves();
  const size_t want = (batch + w - 1) / w;
  const size_t cap = (size_t)cus * groups_per_cu(sh.lds_bytes, w);
  sh.groups = (uint32_t)(want < cap ? want : cap);
}

MixShape mix_shape(uint32_t ht_size, size_t batch, uint32_t cus)
{
  MixShape sh;
  sh.stride_tagged = round_up(ht_size * 3u, 16u);
  sh.stride_plain = round_up(ht_size * 2u, 16u);
  // most waves per CU first (workgroups of g waves, as many as fit), then
  // most of them with tags
  uint32_t best_waves = 0, best_tagged = 0;
  sh.tagged = 1;
  sh.plain = 0;
  for (uint32_t g = kLz4MaxWavesPerGroup; g >= 1; --g) {
    if ((size_t)g > batch && g > 1)
      continue;
    for (uint32_t t = g;; --t) {
      const uint32_t lds = t * sh.stride_tagged + (g - t) * sh.stride_plain;
      if (lds <= kLdsPerCu) {
        uint32_t per_cu = groups_by_lds(lds);
        if (per_cu > 8)
          per_cu = 8;
        const uint32_t waves = g * per_cu, tagged = t * per_cu;
        if (waves > best_waves || (waves == best_waves && tagged > best_tagged)) {
          best_waves = waves;
          best_tagged = tagged;
          sh.tagged = t;
          sh.plain = g - t;
        }
        break; // fewer tags in a group of this size cannot be better
      }
      if (t == 0)
        break;
    }
  }
  sh.lds_bytes = sh.tagged * sh.stride_tagged + sh.plain * sh.stride_plain;
  set_groups(sh, batch, cus);
  return sh;
}

// 0: the mix kernel of rounds 1-4 (four lone waves per CU); 1: pairs with tag tables; 2: pairs without.
// Pairs where they are not slower than the lone waves (scripts/sweep_pair.py, profiles/r05_pair_sweep.txt):
// chunks of more than 32 KiB (the walk is what the second wave shares; the rest of a chunk's work is wave
// 0's alone: 32 KiB chunks 415 against 429 GB/s, 64 KiB 466 against 421) and of at most 64 KiB (longer chunks
// take the walk of one wave), and a batch of two rounds or more of the 3 pairs a CU holds (four lone waves
// hold a chunk more: 1000 x 64 KiB 268 against 338 GB/s, 1500: 360 against 338).
// With the tags in the positions (4-byte elements: four pairs per CU, every lone wave with a filter too) pairs win
// from 32 KiB chunks and a thousand chunks on (sweep_pair3.log: 32 KiB 1 121 against 1 052 GB/s, 16 KiB 891 / 880,
// 1000 x 64 KiB 677 / 684, 1500: 738 / 692).
int pair_mode(uint32_t ht_size, size_t max_chunk_bytes, size_t batch, bool inpos, size_t cus, const Lz4Overrides& knobs)
{
  if (knobs.has_pair)
    return ht_size >= 8192 ? knobs.pair : 0;
  return ht_size >= 8192 && max_chunk_bytes <= 65536
                 && (inpos ? max_chunk_bytes > 16384 && batch >= 4u * cus
                           : max_chunk_bytes > 32768 && batch >= 2u * 3u * cus)
             ? 1 : 0;
}

// The pair shape: one chunk per workgroup of two waves; `tags` (0: none, 1: a tag table -- 64 KiB chunks:
// three workgroups per CU instead of four --, 2: in the positions).
void pair_shape(Lz4LdsLaunch& l, uint32_t ht_size, size_t batch, uint32_t tags, uint32_t cus, const Lz4Overrides& knobs)
{
  l.pair_tags = tags;
  l.table_bytes = round_up(ht_size * (tags == 1u ? 3u : 2u), 16u);
  l.lds_bytes = l.table_bytes + kPairSyncBytes;
  if (knobs.pair_lds > l.lds_bytes && knobs.pair_lds <= 64u * 1024u)
    l.lds_bytes = knobs.pair_lds;
  uint32_t per_cu = groups_by_lds(l.lds_bytes);
  if (per_cu > 8)
    per_cu = 8;
  const size_t cap = (size_t)cus * per_cu;
  l.grid = (uint32_t)(batch < cap ? batch : cap);
}

Lz4FarLaunch far_geometry(uint32_t ht_size, uint32_t cls, size_t batch, size_t far_capacity, uint32_t cus,
                          const Lz4Overrides& knobs)
{
  const uint32_t table = 2u * table_entries(ht_size);
  Lz4FarLaunch g = {};
  // lanes a trip of the device-table waves' lean form looks up
  g.span = knobs.span ? knobs.span : cls == kClassDense ? (uint32_t)kFarSpanFull : (uint32_t)kFarSpan;
  if (knobs.slots) { // (that geometry for every far-type launch, as many workgroups as fit a CU)
    g.near = knobs.near;
    g.far = knobs.far;
    g.slots = knobs.slots;
    g.lds_bytes = g.near * (table + 2u * g.slots) + g.far * 2u * g.slots;
    uint32_t per_cu = g.lds_bytes <= kLdsPerCu ? groups_per_cu(g.lds_bytes, g.waves()) : 0;
    g.groups = per_cu * cus;
  } else {
    // few chunks: a wave with its table in LDS for each of them, as far as LDS goes
    const uint32_t lone_lds = table + 2u * kFarScratchSlots;
    const uint32_t lone_per_cu = lone_lds <= kLdsPerCu ? groups_per_cu(lone_lds, 1) : 0;
    if (lone_per_cu > 0 && batch <= (size_t)lone_per_cu * cus) {
      g.near = 1;
      g.far = 0;
      g.slots = kFarScratchSlots;
      g.lds_bytes = lone_lds;
      g.groups = (uint32_t)batch;
      return g;
    }
    // else: workgroups of 1, 2 or 4 LDS-table waves and as many device-table waves as fill the CU's
    // 32 wave slots (dense, wide) or two and a half per LDS-table wave (sparse), as many workgroups per CU as
    // LDS holds -- the split with the most LDS-table waves per CU, then the smallest workgroups
    // (64 KiB chunks: 4 x (1 + 7), sparse 2 x (2 + 5); 8 KiB chunks: 8 x (1 + 3); chunks of 2 KiB: 8 x (4 + 0))
    g.slots = 512;
    uint32_t best = 0, best_near = 0;
    for (uint32_t wn = 1; wn <= 4; wn *= 2)
      for (uint32_t per_cu = 8; per_cu >= 1; --per_cu) {
        if (per_cu * wn > 32)
          continue;
        const uint32_t nf = 32 / per_cu - wn;
        if (wn + nf > (uint32_t)kFarMaxWavesPerGroup)
          continue;
        const uint32_t lds = wn * table + (wn + nf) * 2u * g.slots;
        if (lds <= kLdsPerCu && groups_by_lds(lds) >= per_cu) {
          // (sparse: pairs of LDS-table waves, so that two and a half device-table waves go with each)
          if (per_cu * wn > best_near || (cls == kClassSparse && per_cu * wn == best_near && wn == 2)) {
            best_near = per_cu * wn;
            best = per_cu;
            g.near = wn;
            g.far = nf;
          }
          break; // (fewer workgroups of this kind per CU hold no more LDS tables)
        }
      }
    if (best == 0) { // (tables beyond what LDS holds: device-table waves only)
      g.near = 0;
      g.far = 4;
      g.slots = kFarScratchSlots;
      best = 8;
    }
    // sparse data (text): the device-table waves beyond two and a half per LDS-table wave only queue
    // on the fabric (64 KiB chunks, 65 536 of them, LDS-table + device-table waves per CU: 4 + 8: 55.2
    // GB/s, 4 + 10: 60.7, 4 + 11: 60.4, 4 + 12: 58.2, 4 + 14: 54.8)
    if (cls == kClassSparse && g.near > 0) {
      const uint32_t most = g.near >= 2 ? 5 * g.near / 2 : 3;
      if (g.far > most)
        g.far = most;
    }
    g.groups = best * cus;
  }
  // no more device-table waves than the batch needs and the temp buffer has tables for
  if (g.groups > 0 && g.far > 0) {
    const size_t want = (batch + g.groups - 1) / g.groups; // waves per workgroup that have a chunk
    if (want < g.waves())
      g.far = (uint32_t)(want > g.near ? want - g.near : 0);
    if ((size_t)g.groups * g.far > far_capacity)
      g.far = (uint32_t)(far_capacity / g.groups);
    if (g.near == 0 && g.far == 0)
      g.groups = 0;
  }
  g.lds_bytes = g.near * (table + 2u * g.slots) + g.far * 2u * g.slots;
  if (g.groups > 0 && (size_t)g.groups * g.waves() > batch + g.waves() - 1)
    g.groups = (uint32_t)((batch + g.waves() - 1) / g.waves());
  if (g.lds_bytes > kLdsPerCu)
    g.groups = 0;
  return g;
}

// about 16 KiB of input per ticket, but at least 4 tickets per wave so that the last ones even out the load
uint32_t chunks_per_ticket(size_t all_waves, size_t batch, size_t max_chunk_bytes)
{
  uint32_t per_ticket = 1;
  while (per_ticket < 64 && (size_t)per_ticket * (max_chunk_bytes ? max_chunk_bytes : 1) < 16384
         && (size_t)per_ticket * 2 * 4 * all_waves <= batch)
    per_ticket *= 2;
  return per_ticket;
}

} // namespace

Lz4TempLayout lz4_temp_layout(uint32_t ht_size, size_t batch, unsigned base_mod16, size_t temp_bytes)
{
  Lz4TempLayout t = {kAbsent, kAbsent, kAbsent, kAbsent, 0};
  Part part[kParts];
  temp_parts(ht_size, batch, 0, part);
  // (offsets from the 16-byte boundary at or below the buffer: alignment is of the address)
  const size_t end = base_mod16 + temp_bytes;
  size_t at = align(base_mod16, part[kPartHeader].align);
  if (temp_bytes == 0 || at + part[kPartHeader].bytes > end)
    return t; // (too small for the header: nothing)
  t.header = at - base_mod16;
  at += part[kPartHeader].bytes;
  if (at + part[kPartLists].bytes <= end) {
    t.lists = at - base_mod16;
    at += part[kPartLists].bytes;
    if (at + part[kPartRetry].bytes <= end) {
      t.retry = at - base_mod16;
      at += part[kPartRetry].bytes;
    }
  }
  at = align(at, part[kPartTables].align);
  if (at < end) {
    t.far_tables = at - base_mod16;
    t.far_capacity = (end - at) / (table_entries(ht_size) * sizeof(uint16_t));
  }
  return t;
}

size_t lz4_compress_temp_bytes_used(uint32_t ht_size, size_t batch)
{
  // every part, one table per chunk but no more than the chip holds waves, each with its alignment's worth
  // of room ahead of it
  Part part[kParts];
  temp_parts(ht_size, batch, batch < 8192 ? batch : 8192, part);
  size_t bytes = 0;
  for (const Part& p : part)
    bytes += (p.align > 1 ? p.align : 0) + p.bytes;
  return bytes;
}

Lz4CompressPlan lz4_plan_compress(uint32_t ht_size, size_t batch, int elem_size, size_t max_chunk_bytes, Lz4Mode mode,
                                  uint32_t cus, unsigned base_mod16, size_t temp_bytes, bool placed,
                                  const Lz4Overrides& knobs)
{
  Lz4CompressPlan p = {};
  p.temp = lz4_temp_layout(ht_size, batch, base_mod16, temp_bytes);
  const bool header = p.temp.header != kAbsent;
  p.refused = placed && !header; // (one slot per RESIDENT wave: needs the persistent grids)
  p.routed = header && mode == Lz4Mode::Auto && p.temp.lists != kAbsent;
  if (p.routed) {
    // (chunks per workgroup: one per wave while that leaves the chip room, at most 64 -- one list
    // atomic per workgroup and class, and the atomics of a class all go to one address)
    uint32_t per_group = kRouteWaves;
    while (per_group < kRouteMostPerGroup && batch / per_group > 4096)
      per_group *= 2;
    p.route_per_group = per_group;
    p.route_grid = (uint32_t)((batch + per_group - 1) / per_group);
  }

  // ---- the LDS shape
  Lz4LdsLaunch& l = p.lds;
  MixShape mix = mix_shape(ht_size, batch, cus);
  // 4-byte elements in chunks of at most 64 KiB: the tags live in the positions' two spare bits (lz4_common.hiph,
  // Tables INPOS) -- no tag table, four pairs per CU instead of three, four lone waves all with a filter
  l.inpos = elem_size == 4 && max_chunk_bytes <= 65536 && knobs.inpos;
  const int pmode = pair_mode(ht_size, max_chunk_bytes, batch, l.inpos, cus, knobs);
  pair_shape(l, ht_size, batch, l.inpos ? 2u : pmode == 1 ? 1u : 0u, cus, knobs);
  if (l.inpos) { // (every wave's tables are the position table alone)
    mix.tagged = 0;
    mix.plain = kLz4MaxWavesPerGroup;
    while (mix.plain > 1 && (size_t)mix.plain > batch)
      --mix.plain;
    mix.lds_bytes = mix.plain * mix.stride_plain;
    set_groups(mix, batch, cus);
  }
  l.pair = pmode != 0;
  l.tagged = mix.tagged;
  l.stride_tagged = mix.stride_tagged;
  l.stride_plain = mix.stride_plain;
  // (no header, no ticket counter: no persistent workgroups, one chunk per wave)
  if (l.pair) {
    l.per_ticket = chunks_per_ticket(l.grid, batch, max_chunk_bytes);
    l.waves = 2;
    if (!header)
      l.grid = (uint32_t)batch;
  } else {
    l.per_ticket = chunks_per_ticket((size_t)mix.groups * mix.waves(), batch, max_chunk_bytes);
    l.waves = mix.waves();
    l.lds_bytes = mix.lds_bytes;
    l.grid = header ? mix.groups : (uint32_t)((batch + mix.waves() - 1) / mix.waves());
  }

  // ---- the far classes
  p.forced_far = kClassMix;
  const uint32_t forced = mode == Lz4Mode::Far ? kClassDense : mode == Lz4Mode::FarSparse ? kClassSparse
                          : mode == Lz4Mode::FarWide ? kClassWide : kClassMix;
  for (uint32_t cls = kClassDense; cls <= kClassWide && header; ++cls)
    if (p.routed || cls == forced) {
      Lz4FarLaunch& g = p.far[cls];
      g = far_geometry(ht_size, cls, batch, p.temp.far_tables != kAbsent ? p.temp.far_capacity : 0, cus, knobs);
      if (g.groups)
        g.per_ticket = chunks_per_ticket((size_t)g.groups * g.waves(), batch, max_chunk_bytes);
      if (!p.routed && g.groups)
        p.forced_far = cls;
    }
  return p;
}

Lz4DecompressPlan lz4_plan_decompress(size_t batch, uint32_t cus, unsigned base_mod16, size_t temp_bytes)
{
  Lz4DecompressPlan p = {};
  size_t groups = (batch + kDecompWavesPerBlock - 1) / kDecompWavesPerBlock;
  const size_t resident = (size_t)cus * (32 / kDecompWavesPerBlock);
  const size_t at = align(base_mod16, sizeof(uint32_t)), end = base_mod16 + temp_bytes;
  if (groups > resident && temp_bytes > 0 && at + sizeof(uint32_t) <= end) {
    p.first_word = at - base_mod16;
    p.ticket_words = (end - at) / sizeof(uint32_t);
    groups = resident;
  }
  p.grid = (uint32_t)groups;
  return p;
}

} // namespace hcamd
