// The episode of k_rollout and k_episodes (eg_rollout.hip): the text of the kernel body, included once into each of them — k_rollout<h, k>
// with EG_EPISODE_UNIFORM false, which is the code it was, instruction for instruction (its resource lines are pinned,
// tests/test_refine_resources.py; a shared __forceinline__ template kept the lines but rescheduled the prologue), k_episodes<k> with it
// true.  kUniform: the values that are the same in every lane but that the compiler cannot know to be — the result of a call that is not
// inlined, first of all weighted_pick's — are said to be uniform where they arise (uni()); everything the action loop derives from them
// (the loop's own exit, rng.index, the list lengths and log cursors, phase, status) then stays in scalar registers.
// In scope where this is included: kHelpers, kKind and the kernel's arguments T, S_in, O, seed, first_index, n_episodes, replay_mask,
// replay_period, stats, emap.  No include guard: it is meant to be included twice.
  constexpr bool kUniform = EG_EPISODE_UNIFORM;
  constexpr bool kHeavy = kKind == kReplayLong, kReplay = kKind != kLean;
  constexpr bool kPark = kHeavy && kHelpers == 0 && EG_HEAVY_WAVES >= 4;
  const int lane = threadIdx.x & (kWave - 1);
  if (blockIdx.x >= emap.count) return;
  if constexpr (kReplay) {      // (uniform for the whole grid)
    // (a plan batch launches each variant over exactly the plans it serves: eg_plans.cpp launch_plans)
    const bool long_list = S_in.state()->has_lists && S_in.resident_list_len() > kShortReplayMax;
    if (S_in.plan_pool == nullptr && long_list != kHeavy) return;
    if (emap.hoist_seq != 0ull && *emap.hoist == emap.hoist_seq) return;      // served by k_replay_coop / k_replay_broadcast
    if constexpr (kHeavy) if (emap.solo_seq != 0ull && emap.solo[blockIdx.x] == emap.solo_seq) return;      // done by k_replay_solo
  }
  const uint32_t e = map_episode(emap, blockIdx.x);
  if (e >= n_episodes) return;
  // The tail of a large launch.  A grid of several rounds of waves ends when its last-dispatched episodes do, and those run their last
  // stretch on SIMDs that are emptying (a launch of 16 384 sampled episodes keeps 3.1 of its 4 wave slots per SIMD filled on average,
  // profiles/r04_lean_occupancy.txt).  The episodes dispatched last therefore win issue arbitration over the older waves on their
  // SIMD — which are about to end anyway —, in three steps of 640 workgroups: 16 384 episodes 1.028 -> 1.001 ms, 14 746: 0.942 -> 0.914
  // (profiles/r04_ab_notes.log r04x).  Not for grids that are resident all at once.
  if constexpr (kHelpers == 0) {
    constexpr uint32_t kTailStep = 640u;
    if (emap.count > 8192u) {
      const uint32_t behind = emap.count - 1u - blockIdx.x;      // workgroups dispatched after this one
      if (behind < kTailStep) __builtin_amdgcn_s_setprio(3);
      else if (behind < 2u * kTailStep) __builtin_amdgcn_s_setprio(2);
      else if (behind < 3u * kTailStep) __builtin_amdgcn_s_setprio(1);
    }
  }
  uint32_t search_seq = 0, year_seq = 0;      // commands to the helper wave share one sequence
  PrefixCache prefix_cache0 = {0.0, -1, 0};
  if constexpr (kHelpers > 0) {   // waves 1..kHelpers serve the episode wave's placement searches (see helper_loop)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // (the helper also brings the 8 KB factor table into LDS: it has nothing else to do until the first search, and the
    //  barrier of that search orders its LDS writes before anybody's reads)
    if (wave > 0) { load_latency_tables(T, lane); helper_loop(T, lane, wave); return; }
    __builtin_amdgcn_s_setprio(3);      // the episode wave is the critical path: it wins issue arbitration over helper waves
    // LDS arrives with whatever the previous workgroup on this CU left in it: a stale word that happens to equal a
    // sequence number would read as "result ready".  The flags start at 0 (sequence numbers start at 1); the helper
    // cannot touch them before the first command's barrier, which also orders these writes.
#ifndef EG_TEST_NO_FLAG_INIT
    if (lane == 0) { sm.hflag[0] = 0u; sm.hflag[1] = 0u; sm.yflag = 0u; }
#endif
  }
  DevSnapshot S = S_in;
  load_state(S);
  if constexpr (kReplay) plan_lists(S, e);
  // iteration.rs:34-42: which episodes replay the best strategy comes from the caller's mask or, when the policy lives on
  // the device (the host cannot know whether a best strategy exists yet), from a period over the global episode index
  // (Replay episodes always run the heavy-capable variant — the launch plan sends them there, eg_api.cpp launch_batch —, so
  //  the lean variant carries no replay code at all.)
  const bool replay = kReplay && (replay_mask != nullptr ? replay_mask[e] != 0
                                                        : (replay_period != 0u && S.has_best_actions && (first_index + e) % replay_period == 0ull));
  const int n_existing = T.n_existing;
#ifdef EG_STAMPS
  unsigned long long stamps[32] = {};
  const unsigned long long t_begin = __builtin_readcyclecounter();
  unsigned long long last_ = t_begin;
#endif

#ifdef EG_STAMPS
  if (kHeavy && lane < 8) sm.hdbg[lane >> 2][lane & 3] = 0ull;
#endif
  load_static_tables<(kHelpers == 0 && !kHeavy)>(T, lane, kHelpers == 0 || kHeavy);      // (the heavy variant's field update reads sm.dr / sl.dr16)
  if constexpr (kHelpers == 0 && !kHeavy) sm.gstage[0][lane] = (int)0xC000C000;      // the kept staging row starts as padding (chunk_product)
  // bit y: the existing-plant prefix sums of year y equal those of year y-1, so last year's end-of-year class sums carry over
  const uint32_t carry_mask = (uint32_t)__ballot(lane > 0 && lane < EG_YEARS && T.pre_co2()[lane] == T.pre_co2()[lane - 1] &&
                                                 T.pre_tg()[lane] == T.pre_tg()[lane - 1] && T.pre_ig()[lane] == T.pre_ig()[lane - 1] &&
                                                 T.pre_sg()[lane] == T.pre_sg()[lane - 1]);
  Rng rng;
  // (a plan-edit batch with same_index runs every variant as global episode first_index: the same fallback draws for all of them)
  unsigned long long stream_e = (unsigned long long)e;
  if constexpr (kReplay) if (S_in.plan_pool != nullptr && emap.same_index != 0u) stream_e = 0ull;
  rng_seed(rng, seed + first_index + stream_e, lane);   // simulation.rs:50-53, one stream per episode
  EG_MARKG(16);

  Episode ep;
  ep.ngen = 0; ep.noff = 0; ep.run_pos = 0; ep.def_pos = 0; ep.act_pos = 0; ep.status = EG_EP_OK; ep.bytes = 32ull; ep.chunks = 0; ep.heavy = -1; ep.heavy_classes = 0; ep.heavy_quads = 0;
  if constexpr (kHeavy) if (emap.solo_seq != 0ull) {      // k_replay_solo gave this episode up after it had claimed a field slot: the same slot
    const unsigned long long w = emap.solo[blockIdx.x];
    if ((w >> 21) == emap.solo_seq && ((w >> 20) & 1ull)) ep.heavy = (int)(w & 0xFFFFFull);
  }
  uint8_t* run_log = O.run_log(e);
  uint8_t* def_log = O.def_log(e);
  uint8_t* act_log = O.act_log(e);
  uint16_t* gen_cell = O.gen_cell(e);
  uint16_t* gen_pack = O.gen_pack(e);
  uint16_t* off_pack = O.off_pack(e);
  // the long-replay variant's lists go on in the record beyond the on-chip window (ListTail); the others end there
  const ListTail tail = {(unsigned long long)gen_cell, (unsigned long long)gen_pack, (unsigned long long)off_pack};
  constexpr int kGenCap = kHeavy ? EG_MAX_GENS : kLdsGens, kOffCap = kHeavy ? EG_MAX_OFFSETS : kLdsGens;
  bool helper_sums = kHelpers > 0;      // (long-replay variant: until a list outgrows the window — the helper only reads LDS)

  // Wave-uniform doubles that are written once a year and read once a year live in LDS, not in (64-lane) registers:
  // sm.acc[0..2] accumulators of metrics_calculation.rs:133-153, [3..6] last yearly row; sm.yend[0..5] last year's
  // end-of-year capital sums (generators, offsets) and CO2 / output class sums; sm.ystate the state the year started in
  if (lane < 8) sm.acc[lane] = 0.0;
  if (lane < 6) sm.yend[lane] = 0.0;

  // The policy row block of a year (128 doubles, + the stalled sampler's tables) goes to LDS at the start of that year.  The
  // small-batch kernel requests it a year ahead — a lone latency-bound wave with registers to spare.  The throughput kernels
  // (kHelpers == 0: 128 registers, four waves per SIMD to hide a latency) request it at the start of its own year, ahead of
  // the year's gathers: held for a year, those seven registers were spilled to scratch and reloaded — the same latency plus
  // the stores.
  constexpr bool kRowAhead = kHelpers > 0;
  double np0 = 0.0, np1 = 0.0;
  if constexpr (kRowAhead) { np0 = S.pol()[lane]; np1 = S.pol()[64 + lane]; }
  const bool stalled = S.stall > 500u;                        // stalled sampler tables travel the same way
  double ns = 0.0; uint8_t nperm = 0;
  if constexpr (kRowAhead) if (stalled) { ns = S.scaled()[lane]; nperm = S.scaled_perm()[lane]; }
  for (int yi = 0; yi < kYears && ep.status == EG_EP_OK; ++yi) {
    const int year = 2025 + yi;
    EG_MARKG(17);
    // ---- requests first: the per-generator / per-offset terms of this year (first 64 of each list).  In the small-batch
    //      kernel the helper wave was asked for this year's sums when last year's actions ended (see below). ----
    const int ngen_s = __builtin_amdgcn_readfirstlane(ep.ngen);
    const int noff_s = __builtin_amdgcn_readfirstlane(ep.noff);
    const bool carry = ((carry_mask >> yi) & 1u) != 0u;
    const bool sums_from_helper = kHelpers > 0 && yi > 0 && (!kHeavy || helper_sums);
    if constexpr (!kRowAhead) {      // this year's policy block: requested first, it lands under the gathers below
      np0 = S.pol()[yi * snap::kPolRow + lane]; np1 = S.pol()[yi * snap::kPolRow + 64 + lane];
      if (stalled) { ns = S.scaled()[yi * 64 + lane]; nperm = S.scaled_perm()[yi * 64 + lane]; }
    }
    YearTerms terms;
    if (!sums_from_helper) terms = year_gather(T, lane, yi, ngen_s, noff_s);
    {  // this year's policy block -> LDS; small-batch kernel: then request next year's
    wave_sync();
    sm.pol[lane] = np0; sm.pol[64 + lane] = np1;
    if (stalled) { sm.scaled[lane] = ns; sm.ydef[128 + lane] = nperm; }
    if constexpr (kRowAhead) if (yi + 1 < kYears) {
      np0 = S.pol()[(yi + 1) * snap::kPolRow + lane]; np1 = S.pol()[(yi + 1) * snap::kPolRow + 64 + lane];
      if (stalled) { ns = S.scaled()[(yi + 1) * 64 + lane]; nperm = S.scaled_perm()[(yi + 1) * 64 + lane]; }
    }
    wave_sync();
    EG_T1(5);
    }
    ep.n_run_y = 0; ep.n_def_y = 0; ep.n_act_y = 0;
    Totals tot; tot.scaled_valid = true;
    EG_TE(14);

    // ---- aggregates at the start of the year (year_gather / year_fold above) ----
    Agg a;
    a.usage = sm.pol[snap::kPolYear + 5];
    a.gcost_prev = sm.yend[0]; a.ocost_prev = sm.yend[1];
    {
      EG_MARKG(18);
      YearSums ys;
      if (sums_from_helper) {      // folded by the helper wave while this wave closed last year
        // (on a timeout the year carries on with whatever the slots hold until the action loop's own status check ends the
        //  episode: a separate way out of the year loop from here cost the small-batch kernel 14 spilled VGPRs)
        for (int spins = 0; __builtin_amdgcn_readfirstlane((int)*(volatile uint32_t*)&sm.yflag) != (int)year_seq; ++spins) {
          __builtin_amdgcn_s_sleep(1);
          if (spins >= kSpinCap) { ep.status = EG_EP_INTERNAL; break; }
        }
        asm volatile("" ::: "memory");
        ys.gcost = sm.ysum[0]; ys.optot = sm.ysum[1]; ys.offs = sm.ysum[2]; ys.ocost = sm.ysum[3];
        ys.co2 = sm.ysum[4]; ys.tg = sm.ysum[5]; ys.ig = sm.ysum[6]; ys.sg = sm.ysum[7]; ys.opcnt = sm.ysum_opcnt;
      } else {
        ys = year_sums_init_current();
#if !defined(EG_PROBE_SKIP) || EG_PROBE_SKIP != 3
        year_fold<kHeavy>(T, lane, yi, ngen_s, noff_s, carry, terms, ys, tail);
#endif
      }
      a.gcost = ys.gcost; a.optot = ys.optot; a.offs = ys.offs; a.ocost = ys.ocost; a.opcnt = ys.opcnt;
      if (carry) { a.co2 = sm.yend[2]; a.tg = sm.yend[3]; a.ig = sm.yend[4]; a.sg = sm.yend[5]; }
      else { a.co2 = ys.co2; a.tg = ys.tg; a.ig = ys.ig; a.sg = ys.sg; }
      EG_T1(0);
    }
    ep.bytes += 2ull * (unsigned long long)(n_existing + ep.ngen) * 56ull + 2ull * (unsigned long long)ep.noff * 8ull + 184ull;

    // ---- the year's actions: phase 0 = deficit repair (simulation.rs:137-141, :319-522),
    //      phase 1 = additional actions (simulation.rs:144-198).  One loop so that apply_action is emitted once. ----
    EG_MARKG(18);
    int replay_idx = 0, replay_def_idx = 0;   // replay_index is keyed per year (sampling.rs:82, :246-247)
    // a replay episode reads this year's lists once: offsets as scalars, the first 128 / 64 entries one per lane (an action is
    // then a v_readlane instead of two dependent global round trips per action)
    int rep_lo = 0, rep_n = 0, repd_lo = 0, repd_n = 0, rep0 = 0, rep1 = 0, repd0 = 0;
    if constexpr (kReplay) if (replay) {
      rep_lo = __builtin_amdgcn_readfirstlane(S.best_off()[yi]); rep_n = __builtin_amdgcn_readfirstlane(S.best_off()[yi + 1]) - rep_lo;
      repd_lo = __builtin_amdgcn_readfirstlane(S.bestd_off()[yi]); repd_n = __builtin_amdgcn_readfirstlane(S.bestd_off()[yi + 1]) - repd_lo;
      if (!S.has_best_actions) rep_n = 0;
      if (!S.has_best_deficit) repd_n = 0;
      rep0 = lane < rep_n ? (int)S.best_actions()[rep_lo + lane] : 0;
      rep1 = kWave + lane < rep_n ? (int)S.best_actions()[rep_lo + kWave + lane] : 0;
      repd0 = lane < repd_n ? (int)S.bestd_actions()[repd_lo + lane] : 0;
    }
    // (the state at the start of the year is only read by the repair loop — most years have no deficit: its division waits for one)
    State year_start;
    year_start.balance = ((a.tg + a.ig) + a.sg) - a.usage;      // state_of(a).balance
    year_start.net = 0.0; year_start.opinion = 0.0; year_start.cost = 0.0;
    int phase = year_start.balance < 0.0 ? 0 : 1;
    if (phase == 0) {
      year_start = state_of(a);
      if (lane == 0) { sm.ystate[0] = year_start.net; sm.ystate[1] = year_start.opinion; sm.ystate[2] = year_start.balance; sm.ystate[3] = year_start.cost; }
    }
    double remaining = -year_start.balance;
    uint32_t attempts = 0, n_add = 0, k_add = 0;
    bool n_add_known = false;
    State cur = year_start;
    EG_TE(15);

    for (int guard = 0; guard < 200000 && ep.status == EG_EP_OK; ++guard) {
      int action;
      if (phase == 0) {
        if (!(remaining > 0.0)) {   // deficit closed: success bonus (simulation.rs:491-519), then go on to phase 1
          const State fin = cur;      // the state after the last repair action (the map has not changed since)
          wave_sync();
          State initial; initial.net = sm.ystate[0]; initial.opinion = sm.ystate[1]; initial.balance = sm.ystate[2]; initial.cost = sm.ystate[3];
          const double success = evaluate_impact(initial, fin);
          if (fin.balance >= 0.0 && success > 0.0 && ep.n_def_y > 0) {
            const double factor = 0.1 * success;
            wave_sync();
            // update_deficit_weights(action_i, factor) for every deficit action of the year, in order (simulation.rs:505-519):
            // factor > 0, so each call only multiplies its own slot and clamps — lane s counts the calls that hit slot s
            // and applies that many multiply-and-clamp steps to dw[s] (the entries do not interact)
            int hits = 0;
            const int mine0 = sm.ydef[lane], mine1 = sm.ydef[64 + lane];      // the year's deficit actions, one per lane
            for (int i = 0; i < ep.n_def_y; ++i) {
              const int da = i < kWave ? __builtin_amdgcn_readlane(mine0, i) : __builtin_amdgcn_readlane(mine1, i - kWave);
              hits += deficit_slot_of(da) == lane ? 1 : 0;
            }
            const double adj = 1.0 + (S.learning_rate * factor * 1.5);
            if (lane < EG_N_DEFICIT && hits > 0) {
              double v = SM_DW[lane];
              for (int k = 0; k < hits; ++k) v = dmin(dmax(v * adj, kMinWeight), kMaxWeight);
              SM_DW[lane] = v;
            }
            wave_sync();
          }
          phase = 1;
          continue;
        }
        attempts += 1;
        EG_MARKG(19);
        if (attempts < 5u) {
          if (replay) {   // sampling.rs:242-313
            if (replay_def_idx < repd_n) {
              action = replay_def_idx < kWave ? __builtin_amdgcn_readlane(repd0, replay_def_idx) : (int)S.bestd_actions()[repd_lo + replay_def_idx];
              replay_def_idx += 1;
            } else action = smart_deficit_fallback(rng, lane);
            if (ep.def_pos >= EG_DEF_CAP || ep.n_def_y >= 128) { ep.status = EG_EP_OVERFLOW; break; }
            if (lane == 0) { def_log[ep.def_pos] = (uint8_t)action; sm.ydef[ep.n_def_y] = (uint8_t)action; }
            ep.def_pos += 1; ep.n_def_y += 1;
          } else action = sample_deficit_weighted<kUniform>(S, rng, tot, lane);
        } else action = 3 * kBattery;   // simulation.rs:369-376
        EG_T1(2);
        if (action >= kFirstOffset) continue;   // only AddGenerator actions are applied in the repair loop (:398)
        // (`cur`, the state before this action, is the state after the previous one: nothing changes the map in between)
      } else {
        if (!n_add_known) {   // simulation.rs:144-187
          n_add_known = true;
          EG_MARKG(24);
          if (replay) {
            n_add = (uint32_t)rep_n;
          } else {   // sampling.rs:380-443
            const uint32_t dcount = (uint32_t)ep.n_def_y;
            const uint32_t cap = dcount >= 20u ? 0u : 20u - dcount;
            if (cap > 0u) {
              const double u = rng_f64(rng, lane);
              if (S.has_cw) {
                const double total = sm.pol[snap::kPolTotCount];   // the count table is never nudged (Q3): its sum is a snapshot constant
                if (total > 0.0) {      // the first count at which the walk reaches <= 0; none: 5 (sampling.rs:406-421)
                  const uint32_t c = (uint32_t)uni<kUniform>(weighted_pick((int)(offsetof(Smem, pol) + 8 * snap::kPolCw), EG_N_COUNTS, u, lane));
                  n_add = c < (uint32_t)EG_N_COUNTS ? (c < cap ? c : cap) : (5u < cap ? 5u : cap);
                }
              } else {   // heuristic branch; min/max actions were evaluated on the host (sampling.rs:425-427)
                const uint32_t hi = S.heur_max < cap ? S.heur_max : cap;
                const uint32_t lo = S.heur_min < hi ? S.heur_min : hi;
                n_add = lo == hi ? lo : lo + rng_range32(rng, lane, hi - lo + 1u);
              }
            }
          }
          EG_T1(2);
        }
        if (k_add >= n_add) break;
        k_add += 1;
        EG_MARKG(19);
        if (replay) {   // sampling.rs:78-145
          if (replay_idx < rep_n) {
            action = replay_idx < kWave ? __builtin_amdgcn_readlane(rep0, replay_idx)
                                        : (replay_idx < 2 * kWave ? __builtin_amdgcn_readlane(rep1, replay_idx - kWave) : (int)S.best_actions()[rep_lo + replay_idx]);
            replay_idx += 1;
          } else action = smart_fallback(rng, lane, year);
          if (ep.run_pos >= EG_RUN_CAP) { ep.status = EG_EP_OVERFLOW; break; }
          if (lane == 0) run_log[ep.run_pos] = (uint8_t)action;
          ep.run_pos += 1; ep.n_run_y += 1;
        } else action = sample_action_weighted<kUniform>(S, rng, tot, lane);
        EG_T1(2);
      }

      // ---- apply_action (actions.rs:40-204), folded into the aggregates ----
      // (the action index is the same in every lane; saying so moves the index arithmetic below to the scalar unit)
      action = __builtin_amdgcn_readfirstlane(action);
      if (action < kFirstOffset) {
        const int t = action / 3, m = action - 3 * t;
        // terms that depend only on (year, type, multiplier) are requested inside the search, right behind its own
        // loads, and land while it runs
        double2 ccv; double cc_prev = 0.0, t12v;
        auto between = [&]() {
          ep.bytes += (unsigned long long)kCells * 8ull + (unsigned long long)(n_existing + ep.ngen) * 16ull;
          ccv = *reinterpret_cast<const double2*>(T.cc() + ((((unsigned)yi * kTypes + t) * kYears + yi) * kMults + m) * 2);
          if (yi > 0) cc_prev = T.cc()[((((unsigned)(yi - 1) * kTypes + t) * kYears + yi) * kMults + m) * 2];
          t12v = T.t12()[(unsigned)yi * kTypes + t];
        };
        EG_MARKG(20);
        double m03v = 0.0;
        int cell = -1;
        bool placed = false;
        // Long-replay variant at four waves per SIMD: the field code below is not inlined, and what is live across a call has to fit
        // beside the callee's registers.  The year's aggregates — thirty-odd registers of uniform doubles — wait in LDS from here until
        // the field update has been issued.
        if constexpr (kPark) {
          wave_sync();
          if (lane == 0) {
            sm.park[0] = a.co2; sm.park[1] = a.tg; sm.park[2] = a.ig; sm.park[3] = a.sg; sm.park[4] = a.optot; sm.park[5] = a.gcost; sm.park[6] = a.ocost;
            sm.park[7] = a.gcost_prev; sm.park[8] = a.ocost_prev; sm.park[9] = a.offs; sm.park[10] = a.usage;
            sm.park[11] = cur.net; sm.park[12] = cur.opinion; sm.park[13] = cur.balance; sm.park[14] = cur.cost; sm.park[15] = remaining;
            sm.park[16] = __hiloint2double(0, a.opcnt);
          }
          wave_sync();
        }
        if constexpr (kHeavy) if (ep.ngen >= kHeavyGens && ep.heavy != -2) {      // a long list: approximate field + exact evaluation of the few candidates
          const unsigned long long slot_bytes = (unsigned long long)(kRadiusClasses * kFieldStride) * 8ull;
          if (ep.heavy == -1) ep.heavy = heavy_claim(T, lane);
          if (ep.heavy >= 0) {
            const int info = __builtin_amdgcn_readfirstlane(sm.type_info[t]);
            const int hv = info & 15, hrc = (info >> 4) & 15;
            const unsigned long long class_addr = (unsigned long long)T.heavy + (unsigned long long)ep.heavy * slot_bytes + (unsigned long long)(hrc * kFieldStride) * 8ull;
            if (!((ep.heavy_classes >> hrc) & 1)) {      // the first search of this radius class: its field joins
              heavy_build_class<(kHelpers > 0)>(class_addr, tail.gen_cell, lane, hrc, throughput_table(info), (info >> 8) & 15, ep.ngen);
              ep.heavy_classes |= 1 << hrc;
              if constexpr (kHelpers > 0) ep.heavy_quads = heavy_pack_list<true>((unsigned long long)(T.base + tab::hv_box), (unsigned long long)(T.base + tab::dr_meta), lane, ep.heavy_classes);
              else {      // the host packed the list of every subset of classes: this episode's is copied (its first eight entries per lane)
                ep.heavy_quads = __builtin_amdgcn_readfirstlane(T.hv_quads()[ep.heavy_classes]);
                wave_sync();
#pragma unroll
                for (int k = 0; k < kBoxLds / kWave; ++k) sh2.box[k * kWave + lane] = T.hv_lists()[ep.heavy_classes * 1024 + k * kWave + lane];
                wave_sync();
              }
            }
#ifdef EG_STAMPS
            const unsigned long long th0 = __builtin_readcyclecounter();
#endif
            const size_t yv = (size_t)(yi * kMaxVariants + hv) * kPsStride, yc = (size_t)(yi * kMaxVariants + hv) * kPcStride;
            const int hr = place_heavy<(kHelpers > 0)>((unsigned long long)(T.ps() + yv), (unsigned long long)(T.pbase() + yc), (unsigned long long)(T.pcell() + yc), class_addr,
                                                        tail.gen_cell, T.size_factor, lane, hrc, throughput_table(info), ep.ngen);
#ifdef EG_STAMPS
            const unsigned long long th1 = __builtin_readcyclecounter();
            stamps[9] += th1 - th0;
#endif
            if (hr >= 0) { cell = hr & 0xFFFF; ep.chunks += hr >> 16; m03v = T.m03()[cell]; placed = true; between(); }
#ifdef EG_STAMPS
            stamps[10] += __builtin_readcyclecounter() - th1;
#endif
          }
        }
        if constexpr (kHeavy) if (!placed && ep.ngen > kLdsGens) {      // the exact scan, for a list beyond the window (place_search walks LDS)
          const int info = __builtin_amdgcn_readfirstlane(sm.type_info[t]);
          const int xr = place_exact_long<(kHelpers > 0)>((unsigned long long)(T.ps() + (size_t)(yi * kMaxVariants + (info & 15)) * kPsStride), tail.gen_cell,
                                                          T.size_factor, lane, (info >> 4) & 15, throughput_table(info), ep.ngen);
          cell = xr < 0 ? -1 : (xr & 0xFFFF);
          if (xr >= 0) { ep.chunks += xr >> 16; m03v = sm.hres[1].m03; }
          placed = true; between();
        }
        if (!placed) {
#ifdef EG_STAMPS
          cell = __builtin_amdgcn_readfirstlane(place_search<kHelpers, (kHelpers == 0 && !kHeavy), (kHelpers == 0 && !kHeavy)>(T, lane, yi, t, ep.ngen, nullptr, &m03v, prefix_cache0, between, ep.chunks, &search_seq, stamps));
          stamps[11] += 1;
#else
          cell = __builtin_amdgcn_readfirstlane(place_search<kHelpers, (kHelpers == 0 && !kHeavy), (kHelpers == 0 && !kHeavy)>(T, lane, yi, t, ep.ngen, nullptr, &m03v, prefix_cache0, between, ep.chunks, &search_seq));
#endif
        }
        EG_T1(1);
        // the field of every class the episode keeps, for the new generator — requested here, ahead of the bookkeeping, so that it is
        // one call region with the search (the aggregates are parked once); eight list entries per lane and call
        if constexpr (kHeavy) if (cell >= 0 && ep.ngen < kGenCap && ep.heavy_classes != 0) {
          const unsigned long long field_addr = (unsigned long long)T.heavy + (unsigned long long)ep.heavy * ((unsigned long long)(kRadiusClasses * kFieldStride) * 8ull);
          ep.chunks += 2 * ep.heavy_quads;      // 256 entries of 8 B read and written per quad = 2 units of 2 KB
          if constexpr (kHelpers > 0) {
            switch (ep.heavy_quads) {      // (uniform)
              case 1: heavy_add<true, 4>(field_addr, lane, cell, 0); break;
              case 2: heavy_add<true, 8>(field_addr, lane, cell, 0); break;
              case 3: heavy_add<true, 12>(field_addr, lane, cell, 0); break;
              default: heavy_add<true, 16>(field_addr, lane, cell, 0); break;
            }
          } else {
            const unsigned long long hv_list = (unsigned long long)(T.hv_lists() + ep.heavy_classes * 1024);
            if (ep.heavy_quads == 1) heavy_add_body<false, 4>(field_addr, hv_list, lane, cell, 0);
            else heavy_add_body<false, 8>(field_addr, hv_list, lane, cell, 0);
            if (ep.heavy_quads == 3) heavy_add_body<false, 4>(field_addr, hv_list, lane, cell, 8);
            else if (ep.heavy_quads >= 4) heavy_add_body<false, 8>(field_addr, hv_list, lane, cell, 8);
          }
        }
        if constexpr (kPark) {
          wave_sync();
          a.co2 = sm.park[0]; a.tg = sm.park[1]; a.ig = sm.park[2]; a.sg = sm.park[3]; a.optot = sm.park[4]; a.gcost = sm.park[5]; a.ocost = sm.park[6];
          a.gcost_prev = sm.park[7]; a.ocost_prev = sm.park[8]; a.offs = sm.park[9]; a.usage = sm.park[10];
          cur.net = sm.park[11]; cur.opinion = sm.park[12]; cur.balance = sm.park[13]; cur.cost = sm.park[14]; remaining = sm.park[15];
          a.opcnt = __double2loint(sm.park[16]);
        }
        if (cell < 0) { ep.status = cell == kSearchLost ? EG_EP_INTERNAL : EG_EP_NO_LOCATION; break; }   // actions.rs:77-89 is unreachable here (Q16)
        EG_MARKG(21);
        if (ep.ngen >= kGenCap) { ep.status = EG_EP_OVERFLOW; break; }
        if (lane == 0) {
          if (!kHeavy || ep.ngen < kLdsGens) {
            sm.gcell[ep.ngen] = (uint16_t)(cell | (t << 12));
            sm.gbm[ep.ngen] = (uint8_t)(yi | (m << 5));
          }
          if constexpr (kHelpers == 0 && !kHeavy) if (ep.ngen < kWave) {      // the searches' staging row, kept (chunk_product)
            const int gi = cell / kGrid;
            sm.gstage[0][ep.ngen] = (gi | ((cell - gi * kGrid) << 16)) << 1;      // (2 gi, 2 gj)
          }
          gen_cell[ep.ngen] = (uint16_t)cell;
          gen_pack[ep.ngen] = (uint16_t)(t | (yi << 4) | (m << 9));
        }
        wave_sync();
        ep.ngen += 1;
        a.gcost += ccv.x;
        if (yi > 0) a.gcost_prev += cc_prev;
        a.co2 += sm.type_co2[t];
        const double out = sm.type_out[t];
        const int cls = (sm.type_info[t] >> 12) & 3;
        if (cls == 1) a.ig += out; else if (cls == 2) a.sg += out; else a.tg += out;
        a.optot += (m03v + t12v) + ccv.y;
        a.opcnt += 1;
        if constexpr (kHelpers > 0) {      // the searches of both waves read the list from here (chunk_product_latency)
          // (the helper may still be evaluating its chunk of the search that just ended: it masks what lies behind the
          //  list it was given, chunk_product_latency<true>, so the new entry may appear under it)
          if (lane == 0 && (!kHeavy || ep.ngen <= kLdsGens)) {
            const int gi = cell / kGrid;
            sl.gpk[ep.ngen - 1] = (4 * gi) | ((4 * (cell - gi * kGrid)) << 16);
          }
        }
        EG_TE(12);
      } else if (action < kFirstOther) {
        EG_MARKG(20);
        const int ot = (action - kFirstOffset) / 3, m = (action - kFirstOffset) - 3 * ot;
        if (ep.noff >= kOffCap) { ep.status = EG_EP_OVERFLOW; break; }
        const uint16_t p = (uint16_t)(ot | (yi << 4) | (m << 9));
        if (lane == 0) { if (!kHeavy || ep.noff < kLdsGens) sm.opack[ep.noff] = p; off_pack[ep.noff] = p; }
        wave_sync();
        ep.noff += 1;
        a.offs += T.offv()[((unsigned)yi * kOffsetTypes + ot) * kYears + yi];
        a.ocost += T.offc()[((unsigned)yi * kOffsetTypes + ot) * kMults + m];
        if (yi > 0) a.ocost_prev += T.offc()[((unsigned)(yi - 1) * kOffsetTypes + ot) * kMults + m];
        EG_TE(13);
      }
      // 57..59 carry an empty generator id (core.rs:117-119): the lookup fails, nothing changes.  60: DoNothing.

      if (phase == 0) {   // simulation.rs:406-486
        if (ep.def_pos >= EG_DEF_CAP || ep.n_def_y >= 128 || ep.run_pos >= EG_RUN_CAP) { ep.status = EG_EP_OVERFLOW; break; }
        if (lane == 0) { def_log[ep.def_pos] = (uint8_t)action; sm.ydef[ep.n_def_y] = (uint8_t)action; run_log[ep.run_pos] = (uint8_t)action; }
        ep.def_pos += 1; ep.n_def_y += 1; ep.run_pos += 1; ep.n_run_y += 1;
        EG_MARKG(22);
        const State nxt = state_of(a);
#if defined(EG_PROBE_SKIP) && EG_PROBE_SKIP == 2      // diagnostic builds only (profiles/r04_ab_notes.log r04zb): what a piece costs in vector instructions
        remaining = -dmin(nxt.balance, 0.0); cur = nxt;
        if (true) continue;
#endif
        // evaluate_action_impact (scoring.rs:46-85) and the emission / cost terms of simulation.rs:420-452 divide the same
        // differences by the same denominators: each quotient is formed once
        const bool net_positive = cur.net > 0.0;
        double q_net = 0.0, q_cost = 0.0;
        if (net_positive || nxt.net < cur.net) q_net = (cur.net - nxt.net) / max_abs_one(cur.net);
        if (!net_positive || nxt.net < 1000.0) { const double cost_change = nxt.cost - cur.cost; q_cost = -cost_change / max_abs_one(cur.cost); }
        double overall;
        if (net_positive) overall = q_net;
        else {
          const double opinion_improvement = (nxt.opinion - cur.opinion) / max_abs_one(cur.opinion);
          const double cost_weight = cur.cost > kMaxCost * 8.0 ? 0.8 : 0.5;
          overall = q_cost * cost_weight + opinion_improvement * (1.0 - cost_weight);
        }
        const double em = nxt.net < cur.net ? q_net : 0.0;
        const double ci = nxt.net < 1000.0 ? q_cost : 0.0;
        const double oi = nxt.cost < kMaxCost * 8.0 ? (nxt.opinion - cur.opinion) / dmax(1.0 - cur.opinion, 0.1) : 0.0;
        const double combined = overall * 0.7 + em * 0.15 + ci * 0.1 + oi * 0.05;
#if !defined(EG_PROBE_SKIP) || EG_PROBE_SKIP != 1
        nudge_after_repair(S, lane, action, combined, overall * 0.5);
#endif
        tot.scaled_valid = false;
        remaining = -dmin(nxt.balance, 0.0);
        cur = nxt;
        EG_T1(3);
      } else {            // simulation.rs:193-197
        if (ep.act_pos >= EG_ACT_CAP || ep.run_pos >= EG_RUN_CAP) { ep.status = EG_EP_OVERFLOW; break; }
        if (lane == 0) { act_log[ep.act_pos] = (uint8_t)action; run_log[ep.run_pos] = (uint8_t)action; }
        ep.act_pos += 1; ep.n_act_y += 1; ep.run_pos += 1; ep.n_run_y += 1;
        EG_MARKG(23);
      }
    }
    if (ep.status != EG_EP_OK) break;
    ep.bytes += 2ull * (unsigned long long)(ep.n_act_y + ep.n_def_y);
    if constexpr (kHelpers > 0 && kHeavy) if (ep.ngen > kLdsGens || ep.noff > kLdsGens) helper_sums = false;
    if constexpr (kHelpers > 0) {      // the lists are final for this year: the helper folds next year's starting sums meanwhile
      if (yi + 1 < kYears && (!kHeavy || helper_sums)) {
        search_seq += 1; year_seq = search_seq;
        if (lane == 0) {
          sm.cmd[search_seq & 1][0] = kCmdYear | (yi + 1) | ((int)((carry_mask >> (yi + 1)) & 1u) << 8) | ((int)((carry_mask >> (yi + 2)) & 1u) << 9);
          sm.cmd[search_seq & 1][1] = ep.ngen | (ep.noff << 16);
        }
        wg_barrier_lds();
      }
    }

    // ---- yearly metrics (metrics_calculation.rs:32-175) ----
    EG_MARKG(25);
#if defined(EG_PROBE_SKIP) && EG_PROBE_SKIP == 4
    if (true) continue;
#endif
    const State s = state_of(a);
    const double gen = (a.tg + a.ig) + a.sg;
    const double credit = s.net >= 0.0 ? 0.0 : (-s.net) * sm.pol[snap::kPolYear + 8];
    const double total_capital = a.gcost + a.ocost;
    const double yearly_capital = yi == 0 ? total_capital : total_capital - (a.gcost_prev + a.ocost_prev);
    double sales = 0.0;
    if (S.enable_energy_sales && s.balance > 0.0) { const double gwh = s.balance * 8.76; sales = gwh * 50000.0; }
    const double yearly_total = yearly_capital + 0.0 + 0.0 - credit - (S.enable_energy_sales ? sales : 0.0);
    wave_sync();
    const double total_cost = yi == 0 ? yearly_total : sm.acc[0] + yearly_total;
    const double total_credit = yi == 0 ? credit : sm.acc[1] + credit;
    const double total_sales = yi == 0 ? sales : sm.acc[2] + sales;
    wave_sync();
    if (lane == 0) {
      sm.acc[0] = total_cost; sm.acc[1] = total_credit; sm.acc[2] = total_sales;
      sm.acc[3] = s.net; sm.acc[4] = s.opinion; sm.acc[5] = total_capital; sm.acc[6] = s.balance;
    }
    if (S.write_yearly && lane == 0) {   // one lane: 21 adjacent 8-byte stores (merged pairwise)
      double* row = O.yearly(e) + yi * EG_YEARLY_FIELDS;
      row[EG_Y_YEAR] = (double)year; row[EG_Y_POP] = sm.pol[snap::kPolYear + 6]; row[EG_Y_USAGE] = a.usage; row[EG_Y_GEN] = gen;
      row[EG_Y_BALANCE] = s.balance; row[EG_Y_OPINION] = s.opinion; row[EG_Y_YEARLY_CAPITAL] = yearly_capital;
      row[EG_Y_TOTAL_CAPITAL] = total_capital; row[EG_Y_INFLATION] = sm.pol[snap::kPolYear + 7]; row[EG_Y_CO2] = a.co2;
      row[EG_Y_OFFSET] = a.offs; row[EG_Y_NET_CO2] = s.net; row[EG_Y_YEARLY_CREDIT] = credit; row[EG_Y_TOTAL_CREDIT] = total_credit;
      row[EG_Y_YEARLY_SALES] = sales; row[EG_Y_TOTAL_SALES] = total_sales; row[EG_Y_ACTIVE_GENS] = (double)a.opcnt;
      row[EG_Y_UPGRADE_COSTS] = 0.0; row[EG_Y_CLOSURE_COSTS] = 0.0;   // identically 0 (simulation.rs:41-42)
      row[EG_Y_YEARLY_TOTAL_COST] = yearly_total; row[EG_Y_TOTAL_COST] = total_cost;
    }
    if (lane == 0) {
      O.n_run(e)[yi] = ep.n_run_y;
      O.n_def(e)[yi] = ep.n_def_y;
      O.n_act(e)[yi] = ep.n_act_y;
    }
    if (lane == 0) { sm.yend[0] = a.gcost; sm.yend[1] = a.ocost; sm.yend[2] = a.co2; sm.yend[3] = a.tg; sm.yend[4] = a.ig; sm.yend[5] = a.sg; }
    EG_T1(4);
  }

  wave_sync();
  if (lane == 0) {   // SimulationMetrics, iteration.rs:69-74 (Q2: total_cost is the last year's capital cost)
    O.metrics(e)[0] = sm.acc[3];
    O.metrics(e)[1] = sm.acc[4];
    O.metrics(e)[2] = sm.acc[5];
    O.metrics(e)[3] = sm.acc[6] >= 0.0 ? 1.0 : 0.0;
    *O.status(e) = ep.status;
    *O.n_gens(e) = ep.ngen;
    *O.n_offsets(e) = ep.noff;
    *O.n_draws(e) = (unsigned long long)rng.words;
    *O.bytes_moved(e) = (double)ep.bytes;
    *O.n_chunks(e) = (uint32_t)ep.chunks;
#ifdef EG_STAMPS
    EG_MARKG(26);
    stamps[7] = __builtin_readcyclecounter() - t_begin;
    if constexpr (kHeavy) {      // heavy searches: scan / candidates + records / exact evaluation / field update cycles; chunks, candidates, searches
      stamps[27] = sm.hdbg[0][0]; stamps[28] = sm.hdbg[0][1]; stamps[29] = sm.hdbg[0][2]; stamps[30] = sm.hdbg[0][3];
      stamps[24] = sm.hdbg[1][0]; stamps[25] = sm.hdbg[1][1]; stamps[26] = sm.hdbg[1][2];
    }
    // where did this workgroup run?  HW_ID (se / sh / cu / simd / wave slot) and XCC_ID: more workgroups on one CU than fit
    // at once means some of them had to wait for a slot (second round) — scripts/bench_tail.py
    stamps[31] = (unsigned long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                 ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
    // diagnostic build only: cycle shares go to the (otherwise unread) tail of this episode's act_log buffer
    unsigned long long* dbg = (unsigned long long*)(act_log + EG_ACT_CAP - 256);
    for (int i = 0; i < 32; ++i) dbg[i] = stamps[i];
#endif
  }
  if constexpr (kHelpers > 0) {   // release the helper waves
    search_seq += 1;
    if (lane == 0) {
      sm.cmd[search_seq & 1][0] = -1;
      // after a protocol fault the helper's sequence number cannot be trusted: it finds the exit command in either buffer
      // (it has read the command it is working on into registers, so overwriting that buffer is harmless)
      if (ep.status == EG_EP_INTERNAL) sm.cmd[(search_seq & 1) ^ 1][0] = -1;
    }
    wg_barrier_lds();
  }
  if (stats != nullptr) {   // fused batch-update statistics: this episode's lists are re-read by all lanes
    // The wave re-reads what it stored itself: its stores only have to have left the wave (workgroup-scope release =
    // s_waitcnt vmcnt(0)); they went through to L2 and nothing of these buffers was ever loaded into this CU's L1.  A
    // device-scope fence here would write back and invalidate the XCD's L2 once per episode.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    wave_sync();
    StatsParams P;      // only needed here: not held in registers through the episode
    load_stats_params(S, P);
    episode_update_stats(O, S, P, e, lane, stats, 1ull, emap.stats_rep ? (int)(blockIdx.x % (uint32_t)kStatsReplicas) : -1);
  }
