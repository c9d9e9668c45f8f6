// eg_field.h — placement against a long generator list: the penalty field of a replay episode and the three searches that read it.
// Included by eg_rollout.hip inside its anonymous namespace behind place_search, where this text stood, in both of its objects.  Needs
// from the file in front of it: ChunkBest, chunk_product, chunk_reduce; tail_u16, list_cell; sm, sl, wave_sync, the wave-wide reads
// and maxima, kD2Max.  Called by k_rollout's long-replay variant (eg_rollout.hip), by k_replay_solo / k_replay_lazy
// (eg_replay_solo.h) and by k_heavy_register_budget: the non-inlined functions take the register budget of the tightest launch bound
// among the kernels that reach them, which is why all of these stay in one translation unit.
//
//   load_rec, field_load, factor_by_q, factor_cap     global-memory access by ADDRESS (a pointer that crosses a call loses its address space)
//   heavy_claim, heavy_pack_list                      an episode's field slot; the cells a generator reaches, listed in LDS for the joined classes
//   heavy_add, heavy_build_class                      the eager field: a new generator's factors into every joined class; a class joins
//   exact_product_chain, heavy_exact, heavy_result    the exact evaluation of the candidates a bound leaves
//   place_heavy                                       the search by rank over the approximate scores
//   tiles_refresh, tiles_catch_up_all, place_tiles    the search by tile bounds; kLazy: the field brought up to date only where it is read
//   place_exact_long                                  the exact scan for lists with a tail
//
// Reference (relative to the reference's aiSimulator/src/): gpu/metal_location_search.rs:110-176 — the scores and the arg-max these
// searches reproduce bit for bit; the field itself has no counterpart there.
#pragma once

// ---- heavy episodes: placement against a long generator list --------------------------------------------------------
// The branch-and-bound scan above evaluates whole chunks exactly, O(generators) per chunk.  That is the right trade for
// the 25-45 generators of a sampled episode (2-5 chunks per search), but a replay episode places hundreds (the
// reference's replay records and applies every action twice, SURVEY Q15: 228-468 generators once a replay episode has
// become the best strategy): the best-scoring cells are all taken, the scan goes 15-41 chunks deep, and such an episode
// took 40x the time of a sampled one — a launch lasts as long as its slowest episode.
// From kHeavyGens generators on, an episode keeps in global memory, per radius class it searches for, the product of the
// penalty factors of all its generators for every cell: field[rc][cell] (year-independent; folded in any order, it only
// serves a bound).  A class's field is built when the episode first searches for a type of that class and kept up to date
// from then on.
// A search then is
//   1. approx(c) = ((te * cf) * size) * field[rc][c] over the sorted candidates — one gather and three multiplications
//      per candidate instead of a pass over the generator list — with the same stop rule as the exact scan
//      (field <= 1, so approx(c) <= base(c));
//   2. every candidate with approx >= M * (1 - 2^-30), M the largest approx, is evaluated EXACTLY: the reference's
//      product in list order (exact_product_chain; chunk_product when there are many ties), first maximum in cell order.
// Exactness: exact(c) and approx(c) are both the real product te * cf * size * prod f rounded at most G + 3 times each,
// so they differ by less than 2 (G + 3) 2^-53 < 2^-42 relative while no intermediate is subnormal; the arg-max of the
// exact scores (and every cell tied with it) therefore lies within 2^-41 of M and is among the candidates, and a cell
// below the threshold cannot reach the exact score of M's holder.  Subnormal ranges (M < 1e-250), more than 64
// candidates, or no free field slot fall back to the exact scan above.  Results are the exact scan's, bit for bit.
constexpr int kHeavyGens = 8;       // (the heavy variant only runs replay episodes: their exact scans go deep almost at once)
constexpr int kFieldStride = 2624;                   // doubles per radius class of a field slot
constexpr int kSearchFallback = -3;
// The three functions below are not inlined (they would cost the episode loop its registers), and a pointer that crosses a
// call loses its address space: they take ADDRESSES and make global-memory pointers of them, so that the loads stay
// global_load / global_store instead of flat ones.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const u32x4 __attribute__((address_space(1)))* GlobalVec4;
typedef double __attribute__((address_space(1)))* GlobalF64;
typedef const double __attribute__((address_space(1)))* GlobalF64c;
__device__ __forceinline__ PsRec load_rec(unsigned long long list_addr, int i) {
  const GlobalVec4 p = (GlobalVec4)(list_addr + (unsigned long long)(unsigned)i * sizeof(PsRec));
  const u32x4 lo = p[0], hi = p[1];
  PsRec r;
  __builtin_memcpy(&r, &lo, 16); __builtin_memcpy(reinterpret_cast<char*>(&r) + 16, &hi, 16);
  return r;
}
typedef const int __attribute__((address_space(1)))* GlobalI32c;
__device__ __forceinline__ double field_load(GlobalF64 p) {      // past the CU's L1: the wave wrote this entry itself
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// q: squared cell distance, already capped (kLatency: at kD2Max; otherwise at the class's own cap, table >> 16).  `table`: the
// class's throughput_table() — the small-batch kernel (kLatency) has the full table at a 16-byte stride and goes by `rc`.
template <bool kLatency>
__device__ __forceinline__ double factor_by_q(int rc, int table, int q) {
  if constexpr (kLatency) return sl.dr16[2 * (rc * kD2Stride + q)];
  else return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(&sm) + ((table & 0xFFFF) + q * 8));
}
template <bool kLatency>
__device__ __forceinline__ int factor_cap(int table) { return kLatency ? kD2Max : table >> 16; }
// one slot of the pool for this launch, or -2 (pool exhausted / absent).  The claim word holds launch epoch << 20 | count,
// so no launch has to reset it: the first claim of a launch swaps the new epoch in with a zero count, every claim is then
// ONE fetch-and-add (a compare-and-swap loop here made 1 638 episodes queue behind each other for milliseconds).
__device__ __forceinline__ int heavy_claim(const DevTables& T, int lane) {
  int slot = -2;
  if (lane == 0 && T.heavy != nullptr) {
    unsigned* w = T.heavy_claim;
    const unsigned epoch = T.heavy_epoch & 0xFFFu;
    const unsigned old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((old >> 20) != epoch) atomicCAS(w, old, epoch << 20);      // whoever comes first; a failure means somebody else did it
    const unsigned v = atomicAdd(w, 1u);
    if ((v >> 20) == epoch && (v & 0xFFFFFu) < T.heavy_slots) slot = (int)(v & 0xFFFFFu);
  }
  return __builtin_amdgcn_readfirstlane(slot);
}
// field[rc][c] *= d/R of a generator at `cell`, for every class and every cell closer than the class radius.  The cells
// concerned are the same for every generator up to a translation: the host lists them once (eg_device_tables.cpp, tab::hv_box: 978
// entries {di, dj, squared distance, class} for the reference's six radii, padded to 1024 = 16 per lane) and the heavy
// variant keeps the list in LDS.  One memory round trip: every lane requests its 16 field entries, then multiplies and
// stores.  Entries are distinct, so the order is free.
// There is NO control flow in here, on purpose.  With a branch around every entry (skip cells outside the grid, skip
// classes this episode does not search) the compiler can no longer count which loads are outstanding: it waited for
// vmcnt(0) before every multiplication — that is, for the previous STORE to come back from L2 — and for every list
// entry before the next was requested: 8-12 thousand cycles per generator, measured, for what is one round trip.  So an
// entry that falls outside the grid goes to a spare entry behind its class's cells (kFieldStride > kCells; never read),
// and the padding of the list multiplies a cell no class reaches by exactly 1.0.  Classes the episode keeps no field for
// are not in its list at all: heavy_pack_list rewrites the list in LDS whenever a class joins (bytes count as much as
// round trips here: a thousand and more such episodes share the L2), and the update comes in four lengths.
constexpr int kBoxEntries = 1024;
constexpr uint32_t kBoxPadding = 145u << 10;      // class 0, di = dj = -16, q = 145: a factor of exactly 1.0 (sm.dr is padded with it)
struct __align__(16) SmemHeavy {
  uint32_t box[kBoxEntries];               // di + 16 | (dj + 16) << 5 | q << 10 (9 bits; throughput kernels: place in sm.dr) | class << 19
};
__shared__ SmemHeavy sh;
// Throughput kernel: a copy of the first eight entries per lane only — the list of up to three or four radius classes, the usual case,
// 2 KB: with it the variant stays at nine LDS granules, which still lets sixteen waves share a CU beside the lean grid (eleven granules
// did not) —; entries beyond come from tab::hv_lists itself.
constexpr int kBoxLds = 8 * kWave;
struct __align__(16) SmemHeavyTp { uint32_t box[kBoxLds]; };
__shared__ SmemHeavyTp sh2;
typedef const uint32_t __attribute__((address_space(1)))* GlobalU32c;
// sh.box = the entries of the radius classes in `classes` (the host's list is sorted by class; its words 1024..1030 are where
// each class starts), padded to a multiple of four per lane; returns that multiple (1..4)
// Throughput kernels (!kLatency): the squared distance of an entry is replaced by the entry's place in the compact factor table
// sm.dr (`meta_addr`: tab::dr_meta), so that heavy_add reads the factor without knowing the class's offset and cap.
template <bool kLatency>
__device__ __noinline__ int heavy_pack_list(unsigned long long box_addr, unsigned long long meta_addr, int lane, int classes) {
  const GlobalU32c src = (GlobalU32c)box_addr;
  const GlobalU32c meta = (GlobalU32c)meta_addr;
  auto place = [&](uint32_t en) -> uint32_t {
    if constexpr (kLatency) return en;
    const int rc = (int)(en >> 19), q = (int)((en >> 10) & 511u);
    const int off = (int)meta[rc], cap = (int)meta[8 + rc];
    return (en & ~(511u << 10)) | ((uint32_t)(off + (q < cap ? q : cap)) << 10);
  };
  int n = 0;
  for (int rc = 0; rc < kRadiusClasses; ++rc) {
    if (!((classes >> rc) & 1)) continue;
    const int s0 = __builtin_amdgcn_readfirstlane((int)src[kBoxEntries + rc]), s1 = __builtin_amdgcn_readfirstlane((int)src[kBoxEntries + rc + 1]);
    for (int i = s0 + lane; i < s1; i += kWave) sh.box[n + i - s0] = place(src[i]);
    n += s1 - s0;
  }
  const int padded = (n + 4 * kWave - 1) & ~(4 * kWave - 1);
  for (int i = n + lane; i < padded; i += kWave) sh.box[i] = place(kBoxPadding);
  wave_sync();
  return padded / (4 * kWave);
}
// Throughput kernel: inlined.  A function that is not waits for its stores to be acknowledged before it returns (s_waitcnt vmcnt(0) ahead of
// s_setpc), and waits on entry for whatever its caller had in flight: as a call, the update cost the episode its own loads, then its
// stores' round trip, and before that the cost terms the caller had just requested — three exposed latencies where one is needed.
// `list_addr` (throughput kernel): the entry list of the episode's classes, packed by the host for every subset of classes
// (tab::hv_lists); its first eight entries per lane are in LDS (sh2.box, copied when a class joins).  The small-batch kernel, with LDS
// to spare, packs its own list (sh.box).
template <bool kLatency, int kPerLane>
__device__ __forceinline__ void heavy_add_body(unsigned long long field_addr, unsigned long long list_addr, int lane, int cell, int first) {
#ifdef EG_STAMPS
  const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
  const int gi = cell / kGrid, gj = cell - gi * kGrid;
  const GlobalF64 base = (GlobalF64)field_addr;
  double val[kPerLane], fac[kPerLane]; int off[kPerLane]; uint32_t ens[kPerLane];
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    if constexpr (kLatency) ens[k] = sh.box[(first + k) * kWave + lane];
    else if ((first + k) * kWave < kBoxLds) ens[k] = sh2.box[(first + k) * kWave + lane];      // (`first` is a constant at every call site)
    else ens[k] = ((GlobalU32c)list_addr)[(first + k) * kWave + lane];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (all list entries in one LDS round trip, not one after the other)
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const uint32_t en = ens[k];
    const int ci = gi + (int)(en & 31u) - 16, cj = gj + (int)((en >> 5) & 31u) - 16, rc = (int)(en >> 19);
    const bool inside = (unsigned)ci < (unsigned)kGrid && (unsigned)cj < (unsigned)kGrid;
    fac[k] = factor_by_q<kLatency>(rc, (int)offsetof(Smem, dr), (int)((en >> 10) & 511u));      // (throughput kernels: the entry's place in sm.dr, see heavy_pack_list)
    off[k] = rc * kFieldStride + (inside ? ci * kGrid + cj : kCells);
    val[k] = field_load(base + off[k]);
  }
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) base[off[k]] = val[k] * fac[k];
  // (the stores are left in flight: whoever reads the field next — place_heavy, heavy_build_class — waits for them first)
#ifdef EG_STAMPS
  if (lane == 0) sm.hdbg[0][3] += __builtin_readcyclecounter() - ts0;
#endif
}
template <bool kLatency, int kPerLane>
__device__ __noinline__ void heavy_add(unsigned long long field_addr, int lane, int cell, int first) { heavy_add_body<kLatency, kPerLane>(field_addr, 0ull, lane, cell, first); }
// A class joins: its field = for every cell the product of the factors of the generators placed so far (any order: the
// field only serves a bound).  The field of the 41 blocks of 64 cells sits in registers while the generators pass by; a
// generator only touches the blocks whose rows come within `reach` of its own row (a scalar test per block).
// (`tail_cells`: the cells of the generators beyond the on-chip window, ListTail)
template <bool kLatency>
__device__ __noinline__ void heavy_build_class(unsigned long long class_addr, unsigned long long tail_cells, int lane, int rc, int table, int reach, int ngen) {
  const GlobalF64 f = (GlobalF64)class_addr;
  constexpr int kChunks = (kCells + kWave - 1) / kWave;
  // blocks per pass over the generator list: all of them with registers to spare (small-batch kernel); six passes of seven on the
  // throughput kernel's 72 registers (fourteen per pass spilled 17 of them: with seven the long-replay kernel needs no scratch memory
  // at all) — it happens six times an episode at most
  constexpr int kPer = kLatency ? kChunks : 7;
  const int cap = factor_cap<kLatency>(table);
  const int ngen_s = __builtin_amdgcn_readfirstlane(ngen);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (a field update of the other classes may still be in flight)
#pragma nounroll
  for (int c0 = 0; c0 < kChunks; c0 += kPer) {
    double p[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) p[k] = 1.0;
    for (int gb = 0; gb < ngen_s; gb += kWave) {      // the list in blocks of 64, a generator per lane; then one generator at a time
      const int mine = list_cell(tail_cells, gb, lane, ngen_s, 0);
      const int cnt = ngen_s - gb < kWave ? ngen_s - gb : kWave;
      for (int j = 0; j < cnt; ++j) {
        const int gc = __builtin_amdgcn_readlane(mine, j);
        const int gi = gc / kGrid, gj = gc - gi * kGrid;
        const int row_lo = gi - reach, row_hi = gi + reach;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
          const int ch = c0 + k;      // (uniform; a constant when there is one pass)
          if ((ch * kWave + kWave - 1) / kGrid < row_lo || (ch * kWave) / kGrid > row_hi) continue;      // uniform: scalars against scalars
          const int cell = ch * kWave + lane;
          const int ci = cell / kGrid, cj = cell - ci * kGrid;
          int q = (ci - gi) * (ci - gi) + (cj - gj) * (cj - gj);
          q = q < cap ? q : cap;
          p[k] = p[k] * factor_by_q<kLatency>(rc, table, q);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) { const int cell = (c0 + k) * kWave + lane; if (cell < kCells) f[cell] = p[k]; }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// The reference's product for ONE candidate cell: te times the factor of every generator in list order.  The lanes take a
// generator each for the factors (64 at a time).  A generator at or beyond the radius has the factor 1.0 and x * 1.0 == x
// exactly, so only the generators inside the radius are multiplied in — in list order, as a sequential chain of v_mul_f64
// fed by v_readlane.  The winner of a search is a cell that few generators reach: a handful of multiplications instead
// of one per generator (chunk_product, which evaluates 64 different candidates at once, cannot skip anything).
template <bool kLatency>
__device__ __forceinline__ double exact_product_chain(int rc, int table, int ngen_s, double te, int cell, int lane, unsigned long long tail_cells) {
  const int ci = cell / kGrid, cj = cell - ci * kGrid;
  const int cap = factor_cap<kLatency>(table);
  double s = te;
  for (int gb = 0; gb < ngen_s; gb += kWave) {
    double f = 1.0;
    if (gb + lane < ngen_s) {
      const int gc = list_cell(tail_cells, gb, lane, ngen_s, 0);
      const int gi = gc / kGrid, gj = gc - gi * kGrid;
      int q = (ci - gi) * (ci - gi) + (cj - gj) * (cj - gj);
      q = q < cap ? q : cap;
      f = factor_by_q<kLatency>(rc, table, q);
    }
    unsigned long long near = __ballot(f != 1.0);
    while (near != 0ull) {
      const int j = __ffsll((long long)near) - 1;
      s = s * readlane_f64(f, j);
      near &= near - 1ull;
    }
  }
  return s;
}
// 3. of a search of the field (place_heavy, place_tiles): the exact scores of the candidates — their ranks in sm.gstage[1], `solo_cell` the
//    cell of the only one when the approximate pass has it at hand, else -1 — the reference's product in list order, first maximum in
//    cell order
template <bool kLatency>
__device__ __forceinline__ ChunkBest heavy_exact(unsigned long long list_addr, unsigned long long tail_cells, double size_factor, int lane, int rc, int tbl, int ngen_s,
                                                 int ncand, int solo_cell) {
  ChunkBest b; b.score = 0.0; b.m03 = 0.0; b.cell = kCells;
  if (solo_cell >= 0) {      // the usual case: ONE candidate.  It is the arg-max — the arg-max is among the candidates — and nothing
                             // but its cell is asked for: its exact score (the reference's product over the whole list) need not be
                             // formed at all.  (It is positive: within 2^-42 of an approximate score of at least 1e-250.)
    b.cell = solo_cell; b.score = 1.0;
  } else if (ncand <= 4 || ngen_s > kLdsGens) {      // one at a time, generator-parallel factors and the sequential product (exact_product_chain)
                                                     // (chunk_product below walks the on-chip window only)
    for (int k = 0; k < ncand; ++k) {
      const int rk = __builtin_amdgcn_readfirstlane(sm.gstage[1][k]);
      const PsRec e = load_rec(list_addr, rk);      // the same record in every lane
      const double sk = (exact_product_chain<kLatency>(rc, tbl, ngen_s, e.te, (int)e.cell, lane, tail_cells) * e.cf) * size_factor;
      if (sk > b.score || (sk == b.score && sk > 0.0 && (int)e.cell < b.cell)) { b.score = sk; b.cell = (int)e.cell; b.m03 = e.m03; }
    }
  } else {               // many ties: 64 candidates at once (chunk_product)
    const int r = lane < ncand ? sm.gstage[1][lane] : kCells;
    PsRec e; e.te = 0.0; e.cf = 1.0; e.m03 = 0.0; e.cell = 0u; e.pad = 0u;
    if (r < kCells) e = load_rec(list_addr, r);
    const int table = kLatency ? rc * (kD2Stride * 16) : tbl;
    const double s = chunk_score<kLatency>(table, size_factor, lane, ngen_s, r, e.te, e.cf, (int)e.cell, (int)e.pad);
    b = chunk_reduce<false>(s, (int)e.cell, e.m03);
  }
  return b;
}
// the winner's 0.03 * mean settlement opinion to sm.hres[1].m03; returns cell | chunks requested << 16
__device__ __forceinline__ int heavy_result(const ChunkBest& b, int lane, int K, int ncand) {
  wave_sync();
  if (lane == 0) sm.hres[1].m03 = b.m03;
  wave_sync();
  // requested, in units of 2 KB: K chunks of the compact list (64 x 12 B each), K x 64 field entries of 8 B, and — only when several
  // candidates tie — their full records (the field update that follows bills itself)
  return b.cell | (((3 * K + 7) / 8 + (K + 3) / 4 + (ncand > 1 ? 1 : 0)) << 16);
}
// `list_addr`: the sorted candidate list of (year, variant); `class_addr`: the field of the radius class.
// returns cell | chunks requested << 16, or kSearchFallback (the winner's 0.03 * mean settlement opinion: the caller reads tab::m03)
// The scan reads the compact form of the sorted list, `pb_addr` / `pc_addr` = unpenalised score and cell per rank: three registers per
// chunk in flight instead of the eight of a full record (in the throughput kernel — four waves per SIMD — this function has 72
// registers, k_heavy_register_budget); the full records are only read for candidates that tie.
template <bool kLatency>
__device__ __noinline__ int place_heavy(unsigned long long list_addr, unsigned long long pb_addr, unsigned long long pc_addr, unsigned long long class_addr,
                                        unsigned long long tail_cells, double size_factor, int lane, int rc, int tbl, int ngen) {
#ifdef EG_STAMPS
  const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the last field update's stores are in L2 before anything gathers
  const int ngen_s = __builtin_amdgcn_readfirstlane(ngen);
  constexpr int kChunks = (kCells + kWave - 1) / kWave;      // 41: the list holds exactly kChunks * 64 records
  constexpr int kGroup = 4, kGroups = (kChunks + kGroup - 1) / kGroup;
  constexpr double kKeep = 1.0 - 0x1p-30;
  // 1. largest approximate score M, scanning in descending order of the unpenalised score, four chunks per memory round
  //    trip (the records of the next group are requested while this group's field entries are on their way).  Branch-free per
  //    candidate: a lane keeps its largest approximate score, with the chunk it was seen in written into the value's six lowest
  //    bits (2^-46 relative: far inside the 2^-30 the candidates are kept by; one v_max then keeps value and place) and that
  //    candidate's cell, and its second largest as a value only.  Between rounds only the high words of the lanes' maxima are
  //    reduced — a lower bound of M, within 2^-20: the stop rule scans a little further at most —, the full maximum once at the end.
  //    Should a lane's second largest too end up within 2^-30 of M (ties en masse), pass 2 collects the candidates.
  double M = 0.0; int K = 0;
  double lm = 0.0, l2 = 0.0; int lcell = 0;
  // (the addresses are the same in every lane: as scalar registers they leave every request a 32-bit lane offset — the 72 registers of
  //  this function have no room for an address pair per request)
  auto uniform_u64 = [](unsigned long long a) { return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)a); };
  const unsigned long long pb_s = uniform_u64(pb_addr), pc_s = uniform_u64(pc_addr), a_s = uniform_u64(class_addr);
  auto pb_at = [&](int r) { return *(GlobalF64c)(pb_s + (unsigned long long)((unsigned)r * 8u)); };
  auto pc_at = [&](int r) { return *(GlobalI32c)(pc_s + (unsigned long long)((unsigned)r * 4u)); };
  auto field_at = [&](int cell) { return __hip_atomic_load((GlobalF64)(a_s + (unsigned long long)((unsigned)cell * 8u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  // Two register sets take turns as "this round's records" and "the next round's" (no copies between rounds); the compact lists
  // are padded with zeros far enough (kPcStride) for a round to be requested ahead without asking whether the list has ended.
  static_assert((kGroups + 1) * kGroup * kWave <= kPcStride, "the scan requests a round ahead");
  double cb[kGroup], nb[kGroup]; int cc[kGroup], nc[kGroup];
#pragma unroll
  for (int j = 0; j < kGroup; ++j) { cb[j] = pb_at(j * kWave + lane); cc[j] = pc_at(j * kWave + lane); }
#define EG_SCAN_ROUND(CB, CC, NB, NC, g_)                                                                                        \
  {                                                                                                                              \
    if ((g_) >= kGroups || ((g_) > 0 && !(readlane_f64(CB[0], 0) >= M * kKeep))) break;      /* sorted descending: lane 0 holds the round's bound */ \
    double ap[kGroup];                                                                                                           \
    _Pragma("unroll") for (int j = 0; j < kGroup; ++j) ap[j] = field_at(CC[j]);                                                  \
    _Pragma("unroll") for (int j = 0; j < kGroup; ++j) { NB[j] = pb_at((((g_) + 1) * kGroup + j) * kWave + lane); NC[j] = pc_at((((g_) + 1) * kGroup + j) * kWave + lane); } \
    _Pragma("unroll") for (int j = 0; j < kGroup; ++j) {                                                                         \
      const double v = CB[j] * ap[j];                                                                                            \
      const double key = __hiloint2double(__double2hiint(v), (__double2loint(v) & ~63) | ((g_) * kGroup + j));                   \
      const bool larger = key > lm;                                                                                              \
      l2 = vmax64(l2, vmin64(lm, key));      /* (scores: not negative, finite) */                                                \
      lm = vmax64(lm, key);                                                                                                      \
      lcell = larger ? CC[j] : lcell;                                                                                            \
    }                                                                                                                            \
    M = __hiloint2double((int)wave_max_u32((unsigned)__double2hiint(lm)), 0);      /* (scores are not negative: ordered like their bit patterns) */ \
    K = ((g_) + 1) * kGroup < kChunks ? ((g_) + 1) * kGroup : kChunks;                                                           \
  }
#pragma nounroll
  for (int g = 0;; g += 2) {
    EG_SCAN_ROUND(cb, cc, nb, nc, g)
    EG_SCAN_ROUND(nb, nc, cb, cc, g + 1)
  }
#undef EG_SCAN_ROUND
  M = wave_max_f64(lm);
  if (!(M >= 1e-250)) return kSearchFallback;      // (nothing placeable, or subnormal territory: the exact scan decides)
#ifdef EG_STAMPS
  const unsigned long long ts1 = __builtin_readcyclecounter();
#endif
  // 2. the candidates: everything within 2^-30 of M (as ranks in the sorted list, in sm.gstage[1])
  const double thr = M * kKeep;
  int ncand = 0, solo = -1;      // solo: the lane that holds the only candidate
  if (__ballot(l2 >= thr) == 0ull) {      // (thr > 0) no lane has seen two: the candidates are the lanes' own maxima
    const unsigned long long m1 = __ballot(lm >= thr);
    ncand = __popcll(m1);
    if (ncand == 1) solo = __ffsll((long long)m1) - 1;
    if ((m1 >> lane) & 1ull) sm.gstage[1][__popcll(m1 & ((1ull << lane) - 1ull))] = (__double2loint(lm) & 63) * kWave + lane;
  } else {
    for (int k = 0; k < K; ++k) {
      const double approx = pb_at(k * kWave + lane) * field_at(pc_at(k * kWave + lane));
      const unsigned long long m = __ballot(approx >= thr && approx > 0.0);
      if (m != 0ull) {
        const int pos = ncand + __popcll(m & ((1ull << lane) - 1ull));
        if (((m >> lane) & 1ull) && pos < kWave) sm.gstage[1][pos] = k * kWave + lane;
        ncand += __popcll(m);
      }
    }
  }
  if (ncand > kWave || ncand == 0) return kSearchFallback;
  wave_sync();
  // 3. exact scores of the candidates: the reference's product in list order, first maximum in cell order
#ifdef EG_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long ts2 = __builtin_readcyclecounter();
#endif
  const ChunkBest b = heavy_exact<kLatency>(list_addr, tail_cells, size_factor, lane, rc, tbl, ngen_s, ncand, ncand == 1 && solo >= 0 ? __builtin_amdgcn_readlane(lcell, solo) : -1);
  if (!(b.score > 0.0)) return kSearchFallback;
#ifdef EG_STAMPS
  if (lane == 0) { sm.hdbg[0][0] += ts1 - ts0; sm.hdbg[0][1] += ts2 - ts1; sm.hdbg[0][2] += __builtin_readcyclecounter() - ts2; sm.hdbg[1][0] += (unsigned long long)K; sm.hdbg[1][1] += (unsigned long long)ncand; sm.hdbg[1][2] += 1ull; }
#endif
  return heavy_result(b, lane, K, ncand);
}

// ---- the per-episode replay kernel's search: by tile bounds instead of by rank -----------------------------------------------
// place_heavy walks the candidates in descending unpenalised score.  In a replay the best cells are taken early on, so a search goes
// 8-9 chunks deep in three dependent rounds of gathers: two thirds of the cycles of a replay episode on k_replay_solo, where a lone
// wave pays about ten cycles per instruction.  place_tiles finds the same M by WHERE the cells are: the grid in 7 x 7 tiles of 8 x 8
// cells, and per tile an upper bound of its approximate scores pb(y, c) * field(c).  The unpenalised scores of the years differ by
// population factors only (tab::te: the distance terms are the same every year), so pb(y, c) = r(y, c) * u(c), u(c) the cell's largest
// over the years (tab::ucell) and r(y, c) nearly the same on the whole tile: the bound is rmax(y, tile) * g(tile), rmax the tile's
// largest ratio rounded up (tab::rmax), g an upper bound of u * field on the tile (DevTables::heavy_tiles, per variant).  The field only
// shrinks (every factor is at most 1, and x * f <= x under round-to-nearest), so a bound once true stays true: a field update leaves g
// alone, a variant's first search of an episode starts it at the tile's largest u (tab::umax), and a search writes back the present
// maximum of u * field (rounded up) of every tile it evaluates.  A search
//   1. takes the bounds of the 49 tiles (a lane each) and evaluates the best two: their 128 cells, two per lane, as rows of tab::cbase
//      (the unpenalised score per cell: the doubles tab::pbase holds per rank) and of the field, each cell with place_heavy's key — the
//      high word of pb * field, the low word's six lowest bits replaced by the chunk (rank / 64) its scan meets the cell in;
//   2. evaluates every other tile whose bound is not below hi(M) * (1 - 2^-29), two at a time, M the largest key so far.  A key exceeds
//      its score by less than 64 ulp, so every cell place_heavy would keep (key or score at least M * (1 - 2^-30)) is evaluated.
// What place_heavy's scan reads follows from M.  Its M is the largest key of all cells too (a cell behind the point where it stops has
// a key below the bound it stopped on, and that bound is below the M it had).  It scans groups of four chunks and stops ahead of group
// g > 0 when the group's first unpenalised score pb[256 g] is below hi(M) * (1 - 2^-30), hi(M) the largest key of the groups before
// with its low word cleared.  It cannot stop before group g* = rank(M) / 256 (M itself would be behind the stop), and from the round
// after g* on its hi(M) is the final M's.  So it stops at g_stop, the first g > g* with pb[256 g] < hi(M) * (1 - 2^-30), or at the end
// of the list (kGroups), having read K = min(4 g_stop, 41) chunks: ten group boundaries, one load.  Its candidates lie among the
// cells of rank < 64 K.  It takes its fast path when no lane of its scan (rank % 64) has seen two cells within 2^-30 of M: the
// candidates are then the lanes' largest keys.  place_tiles keeps per lane of its own the largest key with its rank and cell and the
// second largest key; when one of its lanes has seen two, or two candidates share a rank % 64 — ties, which place_heavy resolves on
// its slow path — it returns kTilesUndecided and the caller runs place_heavy.  Otherwise the candidates, their exact evaluation
// (heavy_exact), the fallbacks and the chunks requested are place_heavy's, bit for bit.
// `tab_addr`: the tables (DevTables::base), `yv`: year * kMaxVariants + variant, `tiles_addr`: the variant's 49 tile bounds g
constexpr int kTilesUndecided = -4;
static_assert(kTileW * kTileW == kWave, "a cell of a tile per lane");
constexpr int kNoTile = 63;      // a tile index with no cell on the grid: the second tile of a round that has only one
static_assert(kNoTile >= kTiles && (kNoTile / kTileCols) * kTileW >= kGrid, "kNoTile is off the grid");

// ---- the lazy field (k_replay_lazy: eg_replay_solo.h, DevTables::solo_lazy) ------------------------------------------------------------------
// The eager field is kept current for every cell of every joined class after every placement (heavy_add_body), and built whole when
// a class joins (heavy_build_class) — but a search by tiles reads it in the few tiles it evaluates and nowhere else.  Lazily, a
// placement leaves the field alone, and a tile's 64 values are brought up to date when a search is about to read them: per field
// slot, class and tile a counter `applied` — how many generators of the episode's list the tile's stored values hold (0: none, the
// values are 1.0 whatever is stored: a class joins by zeroing its 49 counters) — in the spare doubles behind the class's cells
// (index kCells is the dump entry of the eager update; the counters, 16 bits each, start at kCells + 1).
// Catching up multiplies the factors of generators applied .. ngen - 1 in, in list order.  The eager value of a cell is
// ((1 * f_1) * f_2) ... over the whole list in list order as well (a generator out of reach contributes exactly 1.0: the table
// holds 1.0 at the cap, and x * 1.0 == x), so what a search reads is the eager field bit for bit — the same multiplications, later.
// A tile nobody evaluates keeps stale, larger values; nothing reads them (place_heavy, which reads by rank, is preceded by
// tiles_catch_up_all), and the tile's bound g is an upper bound of u * field whenever it was taken (the field only shrinks).
constexpr int kTileCounters = kCells + 1;      // (in doubles, class-relative)
static_assert((kFieldStride - kTileCounters) * 8 >= kTiles * 2 && EG_MAX_GENS <= 0xFFFF, "a 16-bit counter per tile fits behind a class's cells");
// `fa`, `fb`: the lane's stored field values of tiles ta, tb (tb may be kNoTile) — on return current, and stored with the tiles'
// counters; `applied`: the class's counters, a tile per lane.  The generators pass by in blocks of 64, one per lane, and are folded the
// way the lean kernel folds a chunk (chunk_product), whose loop is bound by its instruction count as this one is:
//   1. a lane-parallel test finds, per tile, the generators the tile still needs — index at or beyond the tile's counter, inside the
//      list, within `reach` of the tile's box — and those are compacted, in list order, into a staging row per tile: the lane stores
//      its generator's (gi, gj), two int16, at the count of needed generators in the lanes below it.  The rows are Smem::gstage's two:
//      nothing keeps them across a tile round here (place_tiles writes its candidates to row 1 behind its tile loop, heavy_exact's
//      chunk_product stages row 0 anew for every chunk, and the replay kernels' place_search does not keep row 0).  A row of odd
//      length is padded with chunk_product's generator far off the grid; the eight entries behind a row stay that padding.
//   2. a row comes back two generators at a time in one broadcast 64-bit read; per generator factor_at's sequence against the lane's
//      packed cell — packed subtract, dot product, cap, address, table read — and the multiply, in list order.  The two tiles' chains are
//      independent: as long as both rows last, a trip takes a pair of each — four table reads in flight, then the two chains' multiplications
//      interleaved, with the next trip's pairs requested in between.  The longer row's rest follows alone.
//      Pairs, not chunk_product's groups of four with two register sets taking turns: k_replay_lazy keeps its episode in registers across
//      the call of place_tiles, which therefore has the 70 registers it had and no more.  Groups of four of both tiles with two sets made
//      it 120 wide and the kernel spill 36 registers; one set 88 and 8; one set filled in halves 84 and 4; pairs 70 and none (the
//      compiler's resource report each time).  A pair also wastes half a generator's instructions on padding where a group wastes 1.5.
// The same bits as folding every generator into both tiles: the factors are the same table entries by the same squared distances
// (whole cells: the dot product is exact), multiplied in the same order, and every multiplication left out — a generator the tile
// already holds, one beyond the list, one that does not reach the tile's box — is one by the table's 1.0 at the cap, and
// x * 1.0 == x.  A row's padding multiplies by that 1.0.  A lane whose cell is off the grid folds along and stores nothing.
// Per generator and tile that is six vector instructions and half a row read, where the loop it replaces — a readlane and two unpacks
// per generator, then distance, cap, "already held", address, read and multiply per tile — took about fourteen.
// returns the generators folded (one that both tiles need counts once)
static_assert(sizeof(sm.gstage[0]) >= (kWave + 2) * sizeof(int) && sizeof(sm.gstage[0]) % 8 == 0, "a row's padding and read-ahead stay inside the row");
constexpr int kGenPadFar = (int)0xC000C000;      // (chunk_product's: gi = gj = -16384, beyond every cap)
__device__ __forceinline__ int tiles_refresh(unsigned long long a_s, int applied, int ta, int tb, int lane, int rc, int tbl, int reach, int ngen_s,
                                             unsigned long long tail_cells, double& fa, double& fb) {
  (void)rc;
  const int dr_off = tbl & 0xFFFF, cap = factor_cap<false>(tbl);
  const int ra = (ta / kTileCols) * kTileW, ca = (ta % kTileCols) * kTileW, rb = (tb / kTileCols) * kTileW, cb = (tb % kTileCols) * kTileW;
  const int ia = ra + (lane >> 3), ja = ca + (lane & 7), ib = rb + (lane >> 3), jb = cb + (lane & 7);
  const short2v cpa = __builtin_bit_cast(short2v, ia | (ja << 16)), cpb = __builtin_bit_cast(short2v, ib | (jb << 16));      // (small, not negative)
  const int aa = __builtin_amdgcn_readlane(applied, ta), ab = tb < kTiles ? __builtin_amdgcn_readlane(applied, tb) : ngen_s;
  fa = aa == 0 ? 1.0 : fa; fb = ab == 0 ? 1.0 : fb;
  int folded = 0;
  const unsigned span = (unsigned)(kTileW - 1 + 2 * reach);
  const int2* rowa = reinterpret_cast<const int2*>(sm.gstage[0]);
  const int2* rowb = reinterpret_cast<const int2*>(sm.gstage[1]);
  for (int gb = (aa < ab ? aa : ab) & ~(kWave - 1); gb < ngen_s; gb += kWave) {
    const int gc = list_cell(tail_cells, gb, lane, ngen_s, 0), g = gb + lane;
    const int gi = gc / kGrid, gj = gc - gi * kGrid;
    const bool na = g >= aa && g < ngen_s && (unsigned)(gi - ra + reach) <= span && (unsigned)(gj - ca + reach) <= span;
    const bool nb = g >= ab && g < ngen_s && (unsigned)(gi - rb + reach) <= span && (unsigned)(gj - cb + reach) <= span;
    const unsigned long long ma = __ballot(na), mb = __ballot(nb);
    if ((ma | mb) == 0ull) continue;      // (uniform, once a block)
    // 1. the two rows
    const int gp = gi | (gj << 16);
    if (na) sm.gstage[0][__builtin_amdgcn_mbcnt_hi((unsigned)(ma >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ma, 0u))] = gp;
    if (nb) sm.gstage[1][__builtin_amdgcn_mbcnt_hi((unsigned)(mb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mb, 0u))] = gp;
    const int cnt_a = __popcll(ma), cnt_b = __popcll(mb);      // (at most 64: the padding then falls on the row's own tail)
    if (lane == 0) { sm.gstage[0][cnt_a] = kGenPadFar; sm.gstage[1][cnt_b] = kGenPadFar; }
    asm volatile("" ::: "memory");      // LDS executes a wave's accesses in program order: only the compiler must keep it
    folded += __popcll(ma | mb);
    const int pairs_a = (cnt_a + 1) >> 1, pairs_b = (cnt_b + 1) >> 1, both = pairs_a < pairs_b ? pairs_a : pairs_b;
    // 2. both tiles, pair by pair
    if (both > 0) {
      double a0, a1, b0, b1;
      int2 ga = rowa[0], gq = rowb[0];
#pragma nounroll
      for (int k = 0; k < both; ++k) {
        a0 = factor_at(cpa, ga.x, dr_off, cap); b0 = factor_at(cpb, gq.x, dr_off, cap); a1 = factor_at(cpa, ga.y, dr_off, cap); b1 = factor_at(cpb, gq.y, dr_off, cap);
        __builtin_amdgcn_sched_barrier(0);
        ga = rowa[k + 1]; gq = rowb[k + 1];      // (the next trip's, into the registers the addresses have left; behind the last pair: padding, or the row's own tail)
        fa = fa * a0; fb = fb * b0; fa = fa * a1; fb = fb * b1;
      }
    }
    // ... and the rest of the longer row
#define EG_TR_REST(row2, cpk, s, n_pairs)                                                                                          \
    {                                                                                                                              \
      double a0, a1;                                                                                                               \
      int2 gcur = row2[both];                                                                                                      \
      _Pragma("nounroll") for (int k = both; k < n_pairs; ++k) {                                                                   \
        a0 = factor_at(cpk, gcur.x, dr_off, cap); a1 = factor_at(cpk, gcur.y, dr_off, cap);                                        \
        __builtin_amdgcn_sched_barrier(0);                                                                                         \
        gcur = row2[k + 1];                                                                                                        \
        s = s * a0; s = s * a1;                                                                                                    \
      }                                                                                                                            \
    }
    if (pairs_a > both) EG_TR_REST(rowa, cpa, fa, pairs_a)
    else if (pairs_b > both) EG_TR_REST(rowb, cpb, fb, pairs_b)
#undef EG_TR_REST
    asm volatile("" ::: "memory");
  }
  if (ia < kGrid && ja < kGrid) *(GlobalF64)(a_s + (unsigned long long)((unsigned)(ia * kGrid + ja) * 8u)) = fa;
  if (ib < kGrid && jb < kGrid) *(GlobalF64)(a_s + (unsigned long long)((unsigned)(ib * kGrid + jb) * 8u)) = fb;
  if (lane == 0) {
    const GlobalU16 cnt = (GlobalU16)(a_s + 8ull * kTileCounters);
    cnt[ta] = (unsigned short)ngen_s;
    if (tb < kTiles) cnt[tb] = (unsigned short)ngen_s;
  }
  return folded;
}
// every tile of a class current: what a search by rank (place_heavy, after kTilesUndecided) reads.  Slow, and rare.
__device__ __noinline__ void tiles_catch_up_all(unsigned long long class_addr, unsigned long long tail_cells, int lane, int rc, int tbl, int reach, int ngen) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (place_tiles has just stored tiles and counters)
  const int ngen_s = __builtin_amdgcn_readfirstlane(ngen);
  const unsigned long long a_s = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(class_addr >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)class_addr);
  const int applied = lane < kTiles ? tail_u16(a_s + 8ull * kTileCounters, lane) : 0;
  if (__ballot(lane < kTiles && applied != ngen_s) == 0ull) return;
#pragma nounroll
  for (int ta = 0; ta < kTiles; ta += 2) {
    const int tb = ta + 1 < kTiles ? ta + 1 : kNoTile;
    const int ia = (ta / kTileCols) * kTileW + (lane >> 3), ja = (ta % kTileCols) * kTileW + (lane & 7);
    const int ib = (tb / kTileCols) * kTileW + (lane >> 3), jb = (tb % kTileCols) * kTileW + (lane & 7);
    const int ca = ia < kGrid && ja < kGrid ? ia * kGrid + ja : 0, cb = ib < kGrid && jb < kGrid ? ib * kGrid + jb : 0;
    double fa = field_load((GlobalF64)a_s + ca), fb = field_load((GlobalF64)a_s + cb);
    tiles_refresh(a_s, applied, ta, tb, lane, rc, tbl, reach, ngen_s, tail_cells, fa, fb);
  }
}

// `kLazy`: the field is brought up to date tile by tile, here (above); `rc_in` then carries the class's radius in cells too (rc | reach << 8)
template <bool kLazy>
__device__ __noinline__ int place_tiles(unsigned long long tab_addr, int yv, unsigned long long class_addr, unsigned long long tiles_addr,
                                        unsigned long long tail_cells, double size_factor, int lane, int rc_in, int tbl, int ngen) {
  const int rc = kLazy ? rc_in & 255 : rc_in, reach = kLazy ? rc_in >> 8 : 0;
#ifdef EG_STAMPS
  const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the last field update's and search's stores are in L2 before anything reads them
  const int ngen_s = __builtin_amdgcn_readfirstlane(ngen);
  constexpr int kChunks = (kCells + kWave - 1) / kWave, kGroup = 4, kGroups = (kChunks + kGroup - 1) / kGroup;
  constexpr double kKeep = 1.0 - 0x1p-30, kKeepTile = 1.0 - 0x1p-29;
  auto uniform_u64 = [](unsigned long long a) { return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)a); };
  const unsigned long long tab_s = uniform_u64(tab_addr), a_s = uniform_u64(class_addr), t_s = uniform_u64(tiles_addr);
  const unsigned long long yv_s = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(yv);
  const unsigned long long cb_s = tab_s + tab::cbase + yv_s * (8ull * kCells), rk_s = tab_s + tab::crank + yv_s * (2ull * kCells);
  const unsigned long long pb_s = tab_s + tab::pbase + yv_s * (8ull * kPcStride), rm_s = tab_s + tab::rmax + yv_s * (8ull * 64);
  const unsigned long long uc_s = tab_s + tab::ucell + (yv_s % kMaxVariants) * (8ull * kCells);
  const GlobalF64 gmax = (GlobalF64)t_s;
  auto field_at = [&](int cell) { return __hip_atomic_load((GlobalF64)(a_s + (unsigned long long)((unsigned)cell * 8u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto cb_at = [&](int cell) { return *(GlobalF64c)(cb_s + (unsigned long long)((unsigned)cell * 8u)); };
  auto uc_at = [&](int cell) { return *(GlobalF64c)(uc_s + (unsigned long long)((unsigned)cell * 8u)); };
  auto rk_at = [&](int cell) { return (int)*(const uint16_t __attribute__((address_space(1)))*)(rk_s + (unsigned long long)((unsigned)cell * 2u)); };
  // the group boundaries of the sorted list (what place_heavy's stop rule reads), requested now, needed at the end
  const double gb = lane >= 1 && lane < kGroups ? *(GlobalF64c)(pb_s + (unsigned long long)((unsigned)(lane * kGroup * kWave) * 8u)) : 0.0;
  // 1. the bounds, and the two best tiles
  const double bound = lane < kTiles ? *(GlobalF64c)(rm_s + (unsigned long long)((unsigned)lane * 8u)) * field_load(gmax + lane) : 0.0;
  int applied = 0;      // (kLazy) the class's tile counters, in the bounds' round trip; a search evaluates a tile once, so they hold for all of it
  if constexpr (kLazy) applied = lane < kTiles ? tail_u16(a_s + 8ull * kTileCounters, lane) : 0;
  unsigned long long left = __ballot(bound > 0.0);      // tiles not evaluated yet that may hold a positive score
  if (left == 0ull) return kSearchFallback;             // (place_heavy's M: below 1e-250)
  const unsigned hb = (unsigned)__double2hiint(bound);
  const unsigned h1 = wave_max_u32(hb);
  int ta = __ffsll((long long)(left & __ballot(hb == h1))) - 1, tb = kNoTile;
  {
    const unsigned long long rest = left & ~(1ull << ta);
    const unsigned h2 = wave_max_u32(lane == ta ? 0u : hb);
    const unsigned long long second = rest & __ballot(hb == h2);
    if (rest != 0ull) tb = __ffsll((long long)(second != 0ull ? second : rest)) - 1;
  }
  // 2. the tiles, two at a time: per lane the largest key (with its rank and cell) and the second largest
  double lm = 0.0, l2 = 0.0;
  int lrank = 0, lcell = -1;
#ifdef EG_STAMPS
  int tiles = 0;
#endif
  auto fold = [&](double v, int r, int c) {
    const double key = __hiloint2double(__double2hiint(v), (__double2loint(v) & ~63) | (r >> 6));
    const bool larger = key > lm;
    l2 = vmax64(l2, vmin64(lm, key));      // (scores: not negative, finite)
    lm = vmax64(lm, key);
    lrank = larger ? r : lrank; lcell = larger ? c : lcell;
  };
#pragma nounroll
  for (;;) {
    left &= ~(1ull << ta) & ~(1ull << tb);
    const int ia = (ta / kTileCols) * kTileW + (lane >> 3), ja = (ta % kTileCols) * kTileW + (lane & 7);
    const int ib = (tb / kTileCols) * kTileW + (lane >> 3), jb = (tb % kTileCols) * kTileW + (lane & 7);
    const bool ina = ia < kGrid && ja < kGrid, inb = ib < kGrid && jb < kGrid;
    const int ca = ina ? ia * kGrid + ja : 0, cb = inb ? ib * kGrid + jb : 0;      // (a lane off the grid reads cell 0 and scores 0)
    double fa = field_at(ca), fb = field_at(cb);
    const double pa = cb_at(ca), pb = cb_at(cb), ua = uc_at(ca), ub = uc_at(cb);
    const int ra = rk_at(ca), rb = rk_at(cb);
    if constexpr (kLazy) {      // the two tiles' field values current before the keys are formed
      const int folded = tiles_refresh(a_s, applied, ta, tb, lane, rc, tbl, reach, ngen_s, tail_cells, fa, fb);
#ifdef EG_STAMPS
      if (lane == 0) sm.hdbg[0][3] += (unsigned long long)folded;      // (free in lazy mode: heavy_add_body's cycles otherwise)
#else
      (void)folded;
#endif
    }
    fold(ina ? pa * fa : 0.0, ra, ca);
    fold(inb ? pb * fb : 0.0, rb, cb);
    // the tiles' present maxima of u * field, rounded up within their high word: their g from now on
    const unsigned gha = wave_max_u32(ina ? (unsigned)__double2hiint(ua * fa) : 0u), ghb = wave_max_u32(inb ? (unsigned)__double2hiint(ub * fb) : 0u);
    if (lane == 0) {
      gmax[ta] = __hiloint2double((int)gha, -1);
      if (tb < kTiles) gmax[tb] = __hiloint2double((int)ghb, -1);
    }
#ifdef EG_STAMPS
    tiles += tb < kTiles ? 2 : 1;
#endif
    const double m_lo = __hiloint2double((int)wave_max_u32((unsigned)__double2hiint(lm)), 0);      // (a lower bound of M)
    left &= __ballot(bound >= m_lo * kKeepTile);
    if (left == 0ull) break;
    ta = __ffsll((long long)left) - 1;
    const unsigned long long rest = left & (left - 1ull);
    tb = rest != 0ull ? __ffsll((long long)rest) - 1 : kNoTile;
  }
  const double M = wave_max_f64(lm);
  if (!(M >= 1e-250)) return kSearchFallback;      // (nothing placeable, or subnormal territory: the exact scan decides)
#ifdef EG_STAMPS
  const unsigned long long ts1 = __builtin_readcyclecounter();
#endif
  const double thr = M * kKeep;
  if (__ballot(l2 >= thr) != 0ull) return kTilesUndecided;
  // the chunks place_heavy's scan reads (see above)
  const int gstar = (__double2loint(M) & 63) / kGroup;
  const double m_hi = __hiloint2double(__double2hiint(M), 0);
  const unsigned long long stops = __ballot(lane > gstar && lane < kGroups && !(gb >= m_hi * kKeep));
  const int g_stop = stops != 0ull ? __ffsll((long long)stops) - 1 : kGroups;
  const int K = kGroup * g_stop < kChunks ? kGroup * g_stop : kChunks;
  // the candidates: the lanes' largest keys within 2^-30 of M, among the ranks the scan reads — their ranks in sm.gstage[1]
  const unsigned long long m1 = __ballot(lm >= thr && lrank < K * kWave);
  const int ncand = __popcll(m1);
  if (ncand == 0) return kTilesUndecided;      // (M's own cell is one)
  if (ncand > 1) {      // two in one lane of place_heavy's scan: its slow path
    unsigned long long seen = 0ull;
    for (unsigned long long m = m1; m != 0ull; m &= m - 1ull) {
      const unsigned long long bit = 1ull << (__builtin_amdgcn_readlane(lrank, __ffsll((long long)m) - 1) & 63);
      if (seen & bit) return kTilesUndecided;
      seen |= bit;
    }
  }
  if ((m1 >> lane) & 1ull) sm.gstage[1][__popcll(m1 & ((1ull << lane) - 1ull))] = lrank;
  wave_sync();
#ifdef EG_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long ts2 = __builtin_readcyclecounter();
#endif
  // 3. exact scores of the candidates, as place_heavy evaluates them
  const unsigned long long list_addr = tab_s + tab::ps + yv_s * (sizeof(PsRec) * (unsigned long long)kPsStride);
  const ChunkBest b = heavy_exact<false>(list_addr, tail_cells, size_factor, lane, rc, tbl, ngen_s, ncand, ncand == 1 ? __builtin_amdgcn_readlane(lcell, __ffsll((long long)m1) - 1) : -1);
  if (!(b.score > 0.0)) return kSearchFallback;
#ifdef EG_STAMPS
  if (lane == 0) {
    sm.hdbg[0][0] += ts1 - ts0; sm.hdbg[0][1] += ts2 - ts1; sm.hdbg[0][2] += __builtin_readcyclecounter() - ts2;
    sm.hdbg[1][0] += (unsigned long long)K; sm.hdbg[1][1] += (unsigned long long)ncand; sm.hdbg[1][2] += 1ull; sm.hdbg[1][3] += (unsigned long long)tiles;
  }
#endif
  return heavy_result(b, lane, K, ncand);
}

// The exact scan for a list that has outgrown the on-chip window (long-replay variant; reached when the field path cannot
// decide: no field slot, scores in subnormal territory, ties en masse).  The candidates, their order, the stop rule and the tie
// rule are place_search's; the generators stream past in blocks of 64 (the window from LDS, the rest from the episode's record)
// and every lane folds all of them, in list order, for its own candidate: a v_readlane per generator and chunk.  Slow, and rare.
// returns cell | chunks requested << 16, or -1 (no candidate with a positive score: actions.rs:77-89); the winner's 0.03 * mean
// settlement opinion in sm.hres[1].m03
template <bool kLatency>
__device__ __noinline__ int place_exact_long(unsigned long long list_addr, unsigned long long tail_cells, double size_factor, int lane, int rc, int tbl, int ngen) {
  const int ngen_s = __builtin_amdgcn_readfirstlane(ngen);
  const int cap = factor_cap<kLatency>(tbl);
  constexpr int kChunks = (kCells + kWave - 1) / kWave;
  double best = 0.0, m03w = 0.0; int best_c = kCells, chunks = 0;
  for (int chunk = 0; chunk < kChunks; ++chunk) {
    const int r = chunk * kWave + lane;
    const PsRec c = load_rec(list_addr, r);
    const double base = (c.te * c.cf) * size_factor;      // (te = 0 beyond the 2601 candidates)
    if (chunk > 0 && !(readlane_f64(base, 0) >= best)) break;      // sorted descending: lane 0 holds the chunk's bound
    ++chunks;
    const int ci = (int)c.cell / kGrid, cj = (int)c.cell - ci * kGrid;
    double s = c.te;
    for (int gb = 0; gb < ngen_s; gb += kWave) {
      const int mine = list_cell(tail_cells, gb, lane, ngen_s, 0);
      const int cnt = ngen_s - gb < kWave ? ngen_s - gb : kWave;
      for (int j = 0; j < cnt; ++j) {
        const int gc = __builtin_amdgcn_readlane(mine, j);
        const int gi = gc / kGrid, gj = gc - gi * kGrid;
        int q = (ci - gi) * (ci - gi) + (cj - gj) * (cj - gj);
        q = q < cap ? q : cap;      // (the table holds 1.0 there, and x * 1.0 == x)
        s = s * factor_by_q<kLatency>(rc, tbl, q);
      }
    }
    s = (s * c.cf) * size_factor;
    s = r < kCells ? s : 0.0;
    if (__any(s > best || (s == best && s > 0.0 && (int)c.cell < best_c))) {
      const ChunkBest b = chunk_reduce<false>(s, (int)c.cell, c.m03);
      if (b.score > best || (b.score == best && b.cell < best_c)) { best = b.score; best_c = b.cell; m03w = b.m03; }
    }
  }
  wave_sync();
  if (lane == 0) sm.hres[1].m03 = m03w;
  wave_sync();
  return best > 0.0 ? (best_c | (chunks << 16)) : -1;
}
