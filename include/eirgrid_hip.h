/*
 * eirgrid_hip.h — C ABI of the MI355X-native rollout engine (libeirgrid_hip.so).
 *
 * Drop-in boundary for the hot path of ETM-Code/eirgrid's aiSimulator.  The reference has no FFI of its own;
 * each entry point below names the Rust item it replaces (paths relative to aiSimulator/src/):
 *
 *   eg_create / eg_destroy      Map::new + initialize_map              utils/map_handler.rs:351-399, main.rs:74-193
 *   eg_rollout_batch            run_iteration, batched over episodes   core/iteration.rs:10-20 (callers:
 *                                                                       core/multi_simulation.rs:472, :690)
 *   eg_find_suitable_location   MetalLocationSearch::find_suitable_location   gpu/metal_location_search.rs:96-103
 *   eg_place                    the same search as the rollout kernels run it (generators on the 1 km grid), for parity tests
 *   eg_policy_*                 ActionWeights::{new, update_*, apply_*}        ai/learning/weights/ (all files)
 *   eg_policy_apply_episode     the write-locked section               core/multi_simulation.rs:494-508
 *   eg_train_step, eg_policy_push / eg_device_step / eg_policy_pull    the body of the training loop (one batch of
 *                               iterations + the update), on the host or entirely on the device   multi_simulation.rs:425-508
 *   eg_policy_save_json / load_json / append_weight_history / export_improvement_csv
 *                               checkpoints and run-directory files    ai/learning/weights/serialization.rs,
 *                                                                       multi_simulation.rs:166-207, utils/csv_export.rs:155-207
 *
 * Conventions: plain pointers and sizes, caller-allocated host buffers unless a parameter is named d_* (device
 * pointer).  Every function returning int32_t returns EG_OK (0) or a negative EG_ERR_* code; eg_last_error()
 * gives the text.  One eg_ctx per device; a ctx is not thread-safe, independent ctxs may be used from separate
 * host threads.  The library fails loudly (EG_ERR_NO_DEVICE) when no HIP device is present: there is no CPU
 * fallback behind this ABI.
 *
 * Canonical action indices (the reference walks std::HashMap in hash order; this ABI fixes the insertion order
 * of ActionWeights::new, ai/learning/weights/core.rs:35-120):
 *   0..44   AddGenerator(type = idx/3 in models/generator.rs:11-36 order, cost multiplier {100,120,150}[idx%3])
 *   45..56  AddCarbonOffset({Forest, Wetland, ActiveCapture, CarbonCredit}[(idx-45)/3], {100,120,150}[(idx-45)%3])
 *   57 UpgradeEfficiency("")   58 AdjustOperation("",0)   59 CloseGenerator("")   60 DoNothing
 * Deficit table (core.rs:130-152): GasPeaker, GasCombinedCycle, BatteryStorage, PumpedStorage, Biomass,
 *   OnshoreWind, OffshoreWind, UtilitySolar, HydroDam, Nuclear, DomesticSolar, CommercialSolar, TidalGenerator,
 *   WaveEnergy, DoNothing.
 */
#ifndef EIRGRID_HIP_H
#define EIRGRID_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EG_YEARS 26
#define EG_N_ACTIONS 61
#define EG_N_DEFICIT 15
#define EG_N_COUNTS 21
#define EG_N_TYPES 15
#define EG_GRID 51
#define EG_CELLS (EG_GRID * EG_GRID)
#define EG_YEARLY_FIELDS 21

/* Per-episode capacities of the records (an episode that exceeds one ends with status EG_EP_OVERFLOW).  The reference's lists
 * are Vecs (core/simulation.rs:146-162, :406-409; ai/learning/weights/sampling.rs:93-101, :258-266); a replay episode records and
 * applies every action twice, so the lists of a training loop double with every replay episode that becomes the
 * best strategy.  Episodes that replay a long best list (more than 96 actions) run a kernel variant whose lists continue in the
 * episode's own record beyond the on-chip window, up to these capacities — the same 4096 the CPU oracle stops at
 * (oracle/eg_oracle.h OG_LOG_CAP).  Sampled episodes and replays of a short list stay within the on-chip window of
 * EG_ONCHIP_GENS generators / offsets.  The default policy places 25-200; a year adds up to 20 actions, so a policy with its weight
 * on one kind of action places up to 520 generators or 520 offsets: up to and including 512 the oracle's episode bit for bit, beyond
 * it EG_EP_OVERFLOW.  A year's deficit actions are kept up to 128 (the standard world needs 40 at the most; a world of twelve times
 * its demand passes 128 in 2025), beyond that EG_EP_OVERFLOW as well.  tests/test_gpu_capacity_edges.py holds both edges. */
#define EG_MAX_GENS 4096
#define EG_MAX_OFFSETS 4096
#define EG_RUN_CAP 4096
#define EG_DEF_CAP 4096
#define EG_ACT_CAP 4096
#define EG_ONCHIP_GENS 512

#define EG_OK 0
#define EG_ERR_NO_DEVICE (-1)
#define EG_ERR_BAD_ARG (-2)
#define EG_ERR_HIP (-3)
#define EG_ERR_UNSUPPORTED (-4)
#define EG_ERR_NOMEM (-5)
#define EG_ERR_INTERNAL (-6)

#define EG_EP_OK 0
#define EG_EP_OVERFLOW (-1)
#define EG_EP_NO_LOCATION (-2)
#define EG_EP_INTERNAL (-3)      /* the kernel's helper-wave protocol timed out (a defect, never an input property): eg_fetch* report EG_ERR_INTERNAL */
#define EG_EP_INFEASIBLE (-4)    /* a variant of a plan batch that ended EG_EP_OK and violates a plan constraint (eg_plan_constraints_set) */

/* yearly row columns: the scalar fields of YearlyMetrics, analysis/metrics.rs:7-31 */
enum {
  EG_Y_YEAR = 0, EG_Y_POP, EG_Y_USAGE, EG_Y_GEN, EG_Y_BALANCE, EG_Y_OPINION, EG_Y_YEARLY_CAPITAL,
  EG_Y_TOTAL_CAPITAL, EG_Y_INFLATION, EG_Y_CO2, EG_Y_OFFSET, EG_Y_NET_CO2, EG_Y_YEARLY_CREDIT, EG_Y_TOTAL_CREDIT,
  EG_Y_YEARLY_SALES, EG_Y_TOTAL_SALES, EG_Y_ACTIVE_GENS, EG_Y_UPGRADE_COSTS, EG_Y_CLOSURE_COSTS,
  EG_Y_YEARLY_TOTAL_COST, EG_Y_TOTAL_COST
};

typedef struct eg_ctx eg_ctx;
typedef struct eg_policy eg_policy;

/* What initialize_map loads (main.rs:74-193): settlements.json, ireland_generators.csv, coastline_points.json. */
typedef struct {
  int32_t n_settlements;
  const double *settlement_x, *settlement_y;   /* grid metres, clamped to [0, 50000] like data/poi.rs:11-15 */
  const uint32_t *settlement_pop;              /* 2025 population */
  int32_t n_existing;
  const double *existing_x, *existing_y;
  const int32_t *existing_type;                /* generator type index */
  const double *existing_capacity_mw;          /* CSV capacity_mw (data/generators_loader.rs:150-153) */
  int32_t n_coast;
  const double *coast_x, *coast_y;
  int32_t existing_operational_at_start;       /* 0 = reference HEAD: existing plant starts "Planned" in 2024 */
} eg_world;

/* Flags that reach run_simulation (core/simulation.rs:22-31; cli/cli.rs:42-55). */
typedef struct {
  int32_t enable_energy_sales;          /* CLI default true */
  int32_t enable_construction_delays;   /* CLI default false; true is not implemented on the device yet */
  int32_t write_yearly;                 /* 1: fill eg_episode_out.yearly */
} eg_opts;

/* Read-only view of ActionWeights for one batch (ai/learning/weights/mod.rs:50-107). */
typedef struct {
  const double *weights;          /* [26][61] */
  const double *deficit_weights;  /* [26][15] */
  const double *count_weights;    /* [26][21], NULL = absent (dropped by the checkpoint loader) */
  double learning_rate, exploration_rate;
  uint32_t iterations_without_improvement;
  int32_t has_best;
  double best_metrics[4];         /* final_net_emissions, average_public_opinion, total_cost, power_reliability */
  /* replay data (best_actions / best_deficit_actions), flat year-major; NULL when has_best == 0 */
  const int32_t *best_count;          /* [26] */
  const uint8_t *best_actions;        /* sum(best_count) */
  const int32_t *best_deficit_count;  /* [26] */
  const uint8_t *best_deficit_actions;
} eg_policy_snapshot;

/* Host-side result buffers, episode-major.  Any pointer may be NULL (that output is skipped). */
typedef struct {
  double *metrics;      /* [n][4]  SimulationMetrics, core/iteration.rs:69-74 */
  double *yearly;       /* [n][26][21] */
  int32_t *status;      /* [n] EG_EP_* */
  int32_t *n_run;       /* [n][26] current_run_actions per year */
  int32_t *n_def;       /* [n][26] current_deficit_actions per year */
  int32_t *n_act;       /* [n][26] SimulationResult.actions per year */
  uint8_t *run_log;     /* [n][EG_RUN_CAP] flat, year-major */
  uint8_t *def_log;     /* [n][EG_DEF_CAP] */
  uint8_t *act_log;     /* [n][EG_ACT_CAP] */
  int32_t *n_gens;      /* [n] */
  uint16_t *gen_cell;   /* [n][EG_MAX_GENS] placement result: i*51+j on the 1 km grid */
  uint16_t *gen_pack;   /* [n][EG_MAX_GENS] type | build-year index << 4 | multiplier index << 9 */
  int32_t *n_offsets;   /* [n] */
  uint16_t *off_pack;   /* [n][EG_MAX_OFFSETS] offset type | year index << 4 | multiplier index << 9 */
  uint64_t *n_draws;    /* [n] words consumed from the episode stream */
  double *bytes_moved;  /* [n] algorithmic bytes of the episode, SURVEY.md §8(d) formula (bills the whole 2601 x 8 B score field per search) */
  uint32_t *n_chunks;   /* [n] what the episode's placement searches requested from memory, in units of 2 KB: chunks of 64 sorted
                           candidate records (32 B each) — what the branch-and-bound search reads instead of the score field —
                           and, for long (replay) episodes, the entries of their penalty field (eg_field.h place_heavy);
                           bytes touched = bytes_moved - n_gens * 2601 * 8 + n_chunks * 2048 */
} eg_episode_out;

const char *eg_last_error(void);
/* 16 hex digits: sha256 over the sources this library was built from (csrc/Makefile); eirgrid_amd/_native.py compares it
 * with the tree it runs in, so that a stale binary next to edited sources is an import error, not a silent mismatch */
const char *eg_build_hash(void);
int32_t eg_device_count(void);

eg_ctx *eg_create(int32_t device_ordinal, const eg_world *world);
void eg_destroy(eg_ctx *);

/* Run episodes [first_episode_index, first_episode_index + n) against one snapshot.  Episode e draws from
 * StdRng::seed_from_u64(seed + e) (the reference gives every episode the same stream under --seed,
 * core/simulation.rs:50-53; e = 0 reproduces that).  replay_mask[i] != 0 runs episode i with
 * replay_best_strategy = true (core/multi_simulation.rs:461-465).  Results are copied into `out`: the scalar fields and the per-year
 * counts of every episode, and of each list (run_log, def_log, act_log, gen_cell, gen_pack, off_pack) the entries the counts
 * announce — a row's bytes behind the longest list of the batch are not written (they keep what the caller's buffer held). */
int32_t eg_rollout_batch(eg_ctx *, const eg_policy_snapshot *, const eg_opts *, uint64_t seed,
                         uint64_t first_episode_index, uint32_t n_episodes, const uint8_t *replay_mask,
                         eg_episode_out *out);

/* Device-resident variant for the timed path: upload the snapshot once, launch any number of batches (results
 * stay in HBM), then fetch the last batch. */
int32_t eg_upload_snapshot(eg_ctx *, const eg_policy_snapshot *, const eg_opts *);
int32_t eg_rollout_launch(eg_ctx *, uint64_t seed, uint64_t first_episode_index, uint32_t n_episodes,
                          const uint8_t *replay_mask /* host, may be NULL */);
int32_t eg_sync(eg_ctx *);
/* copies the eg_last_batch_size() records of the last launched batch: every non-NULL field of `out` must hold that many */
uint32_t eg_last_batch_size(const eg_ctx *);
int32_t eg_fetch(eg_ctx *, eg_episode_out *out);
/* HIP-event time of the rollout kernel launches since the last call to eg_timing_reset (milliseconds, count). */
int32_t eg_timing_reset(eg_ctx *);
int32_t eg_timing_read(eg_ctx *, double *total_ms, int32_t *n_launches);
/* The same launches seen grid by grid.  A batch with replay episodes is up to three grids on two streams (the replay variants
 * on a side stream, the rest on the null stream): *span_ms = eg_timing_read's total (first start to last end of every batch),
 * *grids_ms = the replay grids' and the lean grid's own durations added up.  Grids that run side by side: span well below the
 * sum; grids that were serialised (e.g. two streams sharing one hardware queue): span == sum. */
int32_t eg_timing_read_grids(eg_ctx *, double *span_ms, double *grids_ms, int32_t *n_launches);
/* Device memory the context holds beyond the 50 KB policy: the world's tables (tab::total, 42 MB: 26 MB of sorted candidate lists, 11.5 MB their compact form, 3.3 MB
 * the per-cell placement prefix the hoisted replay reads), the episode records (one of 41.6 KB per
 * episode of the largest batch so far) and the penalty-field pool of long replay episodes — 126 KB per replay episode of a launch,
 * allocated with the first replay launch unless the host knows the best list to be short (<= 96 actions: it uploaded, rewound or
 * pulled it and no on-device update is in flight), grown to the largest launch since, never beyond
 * EIRGRID_HEAVY_POOL_GB (environment, default 64; an episode without a slot takes the exact scan: slower, same result). */
int32_t eg_memory_report(const eg_ctx *, uint64_t *table_bytes, uint64_t *record_bytes, uint64_t *field_pool_bytes);
/* Batch ("reduced") form of the write-locked update (core/multi_simulation.rs:494-508).
 * eg_update_stats reduces the last launched batch on the device into d_stats (EG_STATS_LEN int64, DEVICE pointer, e.g.
 * a torch tensor): integer sums that do not depend on episode / workgroup / rank order, so ONE sum all-reduce over
 * RCCL is the whole exchange; eg_policy_apply_reduced then applies them on the host.  Layout:
 *   [0] episodes ok  [1] episodes failed  [2] episodes that qualify for contrast learning (learning.rs:160)
 *   [3] NOT a sum: the batch's best score as a sortable integer (bit pattern of the score + 1, 0 = none), a maximum;
 *       used on one GPU to find the best episode inside the update kernel, ignored by every update formula
 *   [8 + y*61 + a]               sum of Q32 ln(penalty_factor), learning.rs:232-239
 *   [8 + 26*61 + y*61 + a]       sum of Q32 ln(mild_penalty),   learning.rs:241-251
 *   [8 + 2*26*61 + y*15 + slot]  deficit actions absent from best_deficit_actions[y], learning.rs:346-352 */
#define EG_STATS_LEN (8 + 2 * EG_YEARS * EG_N_ACTIONS + EG_YEARS * EG_N_DEFICIT)
int32_t eg_update_stats(eg_ctx *, int64_t *d_stats);
/* The timed path fuses all of it: one launch runs the batch, accumulates the statistics in the kernel's epilogue and
 * picks the batch's best episode (highest score, ties to the lowest global index).  `d_packet` (DEVICE pointer,
 * EG_PACKET_BYTES) = int64 stats[EG_STATS_LEN] followed by the candidate record:
 *   f64 score (-1: none) | i64 global index | f64 metrics[4] | i32 n_run[26] | i32 n_def[26] | u8 run_log[EG_RUN_CAP] |
 *   u8 def_log[EG_DEF_CAP]
 * so that one device-to-host copy (after the all-reduce of the stats part when N > 1) feeds eg_policy_apply_reduced. */
#define EG_CANDIDATE_BYTES (8 + 8 + 32 + 4 * EG_YEARS + 4 * EG_YEARS + EG_RUN_CAP + EG_DEF_CAP)
#define EG_PACKET_BYTES (8 * EG_STATS_LEN + EG_CANDIDATE_BYTES)
int32_t eg_rollout_launch_update(eg_ctx *, uint64_t seed, uint64_t first_episode_index, uint32_t n_episodes,
                                 const uint8_t *replay_mask /* host, may be NULL */, void *d_packet);
/* score_metrics of every episode of the last batch (written by eg_update_stats; -1 for failed episodes) */
int32_t eg_fetch_scores(eg_ctx *, double *scores);
/* metrics and action lists of one episode of the last batch (the best-candidate broadcast of SURVEY.md §8(e)) */
int32_t eg_fetch_episode_lists(eg_ctx *, uint32_t episode, double metrics[4], int32_t *n_run, uint8_t *run_log /* EG_RUN_CAP */,
                               int32_t *n_def, uint8_t *def_log /* EG_DEF_CAP */);

/* Full record of ONE episode of the last batch (every non-NULL field of `out`, sized for n = 1). */
int32_t eg_fetch_record(eg_ctx *, uint32_t episode, eg_episode_out *out);
/* The record of the episode that is the policy's best strategy (update_best_strategy, ai/learning/weights/strategy.rs:19-258):
 * with the policy resident on the device, k_apply_update keeps that episode's record next to the policy whenever an
 * update installs a new best strategy.  *state: 0 = no improvement yet, 1 = `out` (n = 1) was filled, 2 = the best
 * episode ran on another rank (ask that rank).  Yearly rows are only meaningful when the policy was pushed with
 * eg_opts.write_yearly = 1.  (NOT the run the reference summarises and exports: that is eg_fetch_best_result below.) */
int32_t eg_fetch_best_run(eg_ctx *, eg_episode_out *out, int32_t *state);

/* The reference's `best_result` (core/multi_simulation.rs:384, :613-620): after its parallel section the reference folds the
 * results of THIS process's iterations in iteration order,
 *     if best_result.map_or(true, |best| evaluate_action_impact(&result.metrics, &best.metrics, optimization_mode) > 0.0)
 *         { best_result = Some(result) }
 * — arguments as written: `result` is the current state, `best` the new one, so a result takes over when the held run is an
 * improvement ON it — and that run is what multi_simulation.rs:821-905 prints and exports (simulation_summary.csv, the detail
 * files).  eg_best_result_track starts the fold at None (mode 1: optimization_mode None, 2: "cost_only" (--cost-only), 0: stop
 * tracking); from then on every batch launched on this context is folded on the device behind its rollout, in global index
 * order, failed episodes skipped (in the reference a failed iteration ends the run).  eg_fetch_best_result copies the held
 * run's record (n = 1; *state 0: none yet, 1: filled; *global_index may be NULL).  One fold per context = per process, as in
 * the reference; eg_evaluate_action_impact is ai/metrics/scoring.rs:46-85 on SimulationMetrics quadruples
 * (metrics_to_action_result, multi_simulation.rs:55-62). */
int32_t eg_best_result_track(eg_ctx *, int32_t mode);
int32_t eg_fetch_best_result(eg_ctx *, eg_episode_out *out, int32_t *state, int64_t *global_index);
double eg_evaluate_action_impact(const double current_metrics[4], const double new_metrics[4], int32_t cost_only);

/* Top-K archive of distinct scenarios (no counterpart in the reference, whose author collected the "Top 10 optimized scenarios" of
 * README.md / mapData/top10/ by hand).  eg_top_k_track(ctx, k, mode) starts an empty archive of 1 <= k <= EG_TOPK_MAX entries (mode 1:
 * optimization_mode None, 2: "cost_only" (--cost-only), 0: stop tracking; the archive stays fetchable); from then on every batch
 * launched on this context is folded into it on the device behind its rollout, where the best_result fold runs.  The archive holds
 * the k highest-ranked DISTINCT SCENARIOS among all episodes folded since tracking started:
 *   rank score   eg_rank_score(metrics, mode): score_metrics of ai/metrics/scoring.rs:5-45 (mode 2: its cost_only branch, :7-15),
 *                evaluated with the shared IEEE-only logarithm of csrc/eg_reduced_math.h, the same bits on the host and the device;
 *   order        score descending, ties to the lower global index;
 *   failures     episodes with status != EG_EP_OK (and a NaN score) are skipped; so is a score of -inf (opinion -inf at or below net zero):
 *                only scores ABOVE -inf can enter, -inf is what the fold's own lists hold for "no candidate";
 *   identity     two episodes are the same scenario when the bit patterns of their 4 metrics AND their 64-bit keys are equal; the key
 *                covers n_act[26] as little-endian int32 followed by act_log[0 .. sum n_act), zero-padded to a multiple of 8 bytes,
 *                read as little-endian 8-byte words w_i:  key = sum_i splitmix64(w_i + i * 0x9E3779B97F4A7C15) mod 2^64, with
 *                splitmix64(z) = z ^ z >> 31 after z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB.
 *                (A collision of keys together with equal metrics would merge two scenarios into one.);
 *   occurrence   a scenario is held once, at its earliest global index, with that episode's whole record (replay episodes of the best
 *                strategy are one scenario, however many batches carry them).
 * The result depends only on the set of episodes folded, not on how they were split into batches, ranks or hoisted replays.  Like
 * best_result the archive lives as long as the context: it is not part of any checkpoint.  eg_fetch_top_k copies the *n_held <= k
 * entries in rank order: `out` rows (sized for k episodes), scores[k] and global_index[k] (either may be NULL).  eg_top_k_track
 * refuses a rank of an eg_group: eg_group_top_k_track folds the ranks' results. */
#define EG_TOPK_MAX 64
int32_t eg_top_k_track(eg_ctx *, int32_t k, int32_t mode);
int32_t eg_fetch_top_k(eg_ctx *, eg_episode_out *out, int32_t *n_held, double *scores, int64_t *global_index);
double eg_rank_score(const double metrics[4], int32_t mode);   /* mode 2: cost_only; 0 or 1: optimization_mode None */

/* Pareto archive: the non-dominated outcomes of everything a run has simulated (no counterpart in the reference, which ranks by one
 * scalar).  eg_pareto_track(ctx, cap, objectives, mode) starts an empty archive of 1 <= cap <= EG_PARETO_MAX entries (cap 0: stop tracking;
 * the archive stays fetchable); from then on every batch launched on this context — eg_rollout_launch / _launch_update / eg_rollout_batch,
 * eg_device_rollout / eg_device_step, eg_train_step — is folded into it on the device behind its rollout, where the best_result and
 * top-K folds run, without host synchronisation.
 *   objectives   metrics[4] = {final_net_emissions, average_public_opinion, total_cost, power_reliability}: lower emissions and cost are
 *                better, higher opinion and reliability are better.  `objectives` is a bit mask, bit i = metric i, 1 <= mask <= 15; only
 *                ACTIVE metrics take part in dominance and identity;
 *   valid        an episode with status EG_EP_OK and none of its four metrics NaN (whatever the mask); invalid episodes are skipped.
 *                Infinities compare as IEEE doubles do, and -0.0 equals +0.0;
 *   dominance    a dominates b when a is at least as good as b in every active metric and strictly better in at least one;
 *   points       two valid episodes are the same POINT when all their active metrics are equal as values.  A point is held once,
 *                represented by the episode with the lowest global index among those folded so far, with that episode's whole record
 *                (the replays of a batch are one entry; no action-record key: the front is a set of outcomes).  An equal point of
 *                lower index folded later takes the entry and its record over; the same index folded twice keeps the held entry;
 *   front        F(S) = the points of S that no point of S dominates.  While nothing has been dropped (n_dropped == 0) the archive is
 *                exactly F(all episodes folded): it depends only on that set — not on how it was split into batches, on their order, or
 *                on the replay hoist;
 *   capacity     after a batch the archive becomes F(held u valid(batch)).  If that has more than cap points, cap of them stay and the
 *                sticky counter n_dropped grows by the number removed (points removed by dominance are not counted).  ONCE n_dropped > 0
 *                THE ARCHIVE IS THE RESULT OF THIS STREAMING RULE AND DEPENDS ON THE BATCH BOUNDARIES: a dropped point no longer
 *                dominates anything.  Which cap points stay is the CAPACITY RULE, chosen with `mode`: the low part of mode picks the
 *                rank score (1: optimization_mode None, 2: cost_only, as for top-K), EG_PARETO_KEEP_SPREAD OR-ed into it picks the
 *                rule — accepted values are 1, 2, 0x101 and 0x102.  Both rules use one ORDER OF PREFERENCE between two entries:
 *                the larger eg_rank_score(metrics, low part of mode) first (a NaN score last), then the lower global index, then the
 *                earlier place in the list (held entries in their order, then the batch's in index order);
 *   keep score   (mode 1 | 2) the first cap points in the order of preference stay: the corner of the front nearest the scalar optimum;
 *   keep spread  (mode 0x101 | 0x102) farthest-point selection on the normalised front.  Let A be the front F(held u valid(batch)) of
 *                more than cap points, and v_i[k] entry i's ORIENTED coordinates: metric k where lower is better, its negation where
 *                higher is better, 0.0 for an inactive metric.
 *                  Normalise.  For each k, lo_k = min_A v[k], hi_k = max_A v[k], r_k = hi_k - lo_k.  If r_k is a finite number > 0,
 *                    u_i[k] = (v_i[k] - lo_k) / r_k: one subtraction and one division, each rounded once.  Otherwise u_i[k] = 0.0 for
 *                    every i: an inactive metric, a metric constant over the front, an infinite metric in the front.
 *                  Distance.  d2(i,j) = ((e0*e0 + e1*e1) + e2*e2) + e3*e3 with e_k = u_i[k] - u_j[k]; every product and every sum is
 *                    rounded on its own (no fused multiply-add).  Squared distances are compared; no square root is taken.
 *                  Selection.  s_0 is the first entry of A in the order of preference: the best-scoring point of the front is never
 *                    dropped, and cap = 1 gives what keep score gives.  Set mind_i = d2(i, s_0).  For r = 1 .. cap-1: s_r is the
 *                    not-yet-selected entry of A with the largest mind, ties by the order of preference; then
 *                    mind_i = min(mind_i, d2(i, s_r)) for all i.
 *                  Result.  s_0 .. s_{cap-1} stay; held entries among them keep their record slots, new ones take the lowest free.
 *                This is greedy k-centre selection: every dropped point lies within max_i mind_i of a kept one;
 *   order        eg_fetch_pareto returns the entries in ascending global index.
 * Plan batches (eg_evaluate_plans, eg_evaluate_plan_edits, the rounds of eg_refine_plan) are not training and are not folded
 * automatically: eg_pareto_fold_last_batch(ctx) folds the last batch, whatever kind it was, on request — episode j of it as global index
 * first_episode_index + j, also in a same_index batch ("which of these 16 384 variants are non-dominated").  EG_ERR_BAD_ARG without
 * tracking or without a batch.  eg_pareto_track refuses, naming the field: a cap outside 0..EG_PARETO_MAX, objectives outside 1..15, a
 * mode other than 1, 2, 0x101 or 0x102 (0, 3, EG_PARETO_KEEP_SPREAD alone, any other bit), a rank of a group — a shard's local front has no bounded message size, so there is no group form.  The
 * archive state and cap record slots (10.6 MB at cap 256) are allocated by eg_pareto_track; like best_result the archive lives as long
 * as the context and is not part of any checkpoint.
 * eg_fetch_pareto copies the *n_held <= cap entries: `out` rows (sized for cap episodes; may be NULL), global_index[cap], scores[cap]
 * (eg_rank_score of each entry), *n_dropped (each may be NULL).
 * Under plan streams (eg_plan_streams_set, below) eg_pareto_fold_last_batch folds what a plan batch left in the records, the committed metrics and status: no other change. */
#define EG_PARETO_MAX 256
#define EG_PARETO_KEEP_SPREAD 0x100     /* OR-ed into the mode of eg_pareto_track, eg_breed_opts, eg_explore_opts, eg_debug_breed_begin: the capacity rule "keep spread" */
int32_t eg_pareto_track(eg_ctx *, int32_t cap, int32_t objectives, int32_t mode);
int32_t eg_pareto_fold_last_batch(eg_ctx *);
int32_t eg_fetch_pareto(eg_ctx *, eg_episode_out *out /* cap rows, may be NULL */, int32_t *n_held, int64_t *global_index /* [cap] or NULL */,
                        double *scores /* [cap] or NULL */, int64_t *n_dropped /* or NULL */);
/* Test hook: eg_debug_load_batch(ctx, metrics, status, NULL, NULL, NULL, n, first_index) (the debug section below), then the batch folded
 * into the Pareto archive as any batch is folded (tracking must be on): crafted metric sets that no rollout will produce. */
int32_t eg_debug_pareto_fold(eg_ctx *, const double *metrics /* [n][4] */, const int32_t *status /* [n] */, uint32_t n, uint64_t first_index);

/* Plan evaluation: what does a given strategy score?  A PLAN is what update_best_strategy installs and a replay episode reads
 * (ai/learning/strategy.rs; sampling.rs:76-145, :240-270): per year a list of canonical action indices 0..60 (best_actions) and the
 * deficit actions, also as canonical indices (best_deficit_actions: an AddGenerator at 100 % or DoNothing), each flat list at most
 * 4 096 entries.  eg_evaluate_plans(ctx, policy, opts, plans, seed, first_episode_index, out) runs plan j as global episode
 * first_episode_index + j: exactly the replay episode (replay_mask = 1) that eg_rollout_batch runs at that index under a snapshot
 * equal to `policy`, except that has_best = 1 and the replay lists are plan j's (both present).  Every other field of the policy is
 * used as given, best_metrics included.  So a replay applies its deficit actions twice; when a year's list runs out the
 * episode goes on with seeded draws from the policy's tables (seed + first_episode_index + j); in-episode nudges are discarded.
 * An evaluation is not training: no statistics, no update packet, no best_result or top-K fold, and the context's resident policy
 * (eg_policy_push / eg_device_step state, eg_fetch_best_run's record, the improvement log) is untouched — the policy goes to a device
 * snapshot of its own.  What it leaves behind is the last batch: eg_last_batch_size() = n_plans and eg_fetch / eg_fetch_record
 * return the plans' records (also copied into `out` when it is not NULL).  Evaluate between whole training steps, never between
 * eg_device_rollout and eg_device_apply.  EG_ERR_BAD_ARG (with a message naming the plan and the field) for n_plans < 1, a NULL
 * pointer, a negative count, counts that do not add up to the *_len of the flat data, an entry >= 61, a list over 4 096 entries;
 * eg_plans_validate runs these checks alone.  A rank of an eg_group is refused (plan batches on a group are not supported).
 *
 * eg_plans_load reads plans from a file in the checkpoint schema (eg_policy_load_json: year-keyed best_actions /
 * best_deficit_actions of SerializableAction; null = empty lists): one JSON document (a checkpoint: one plan) or JSON Lines (one
 * object per non-blank line carrying both keys, optionally "name").  NULL + eg_last_error() on malformed input; the message names
 * every bad line and field.  names[j] is "" when a line has none.  Free with eg_plans_free. */
typedef struct {
  int32_t n_plans;
  const int32_t *best_count;            /* [n][26] */
  const uint8_t *best_actions;          /* plan-major, then year-major: sum(best_count) entries */
  const int32_t *best_deficit_count;    /* [n][26] */
  const uint8_t *best_deficit_actions;  /* sum(best_deficit_count) entries */
  int64_t best_actions_len, best_deficit_actions_len;   /* entries of the two flat arrays */
  const char *const *names;             /* [n] or NULL */
} eg_plan_set;
int32_t eg_plans_validate(const eg_plan_set *);
int32_t eg_evaluate_plans(eg_ctx *, const eg_policy_snapshot *policy, const eg_opts *, const eg_plan_set *, uint64_t seed,
                          uint64_t first_episode_index, eg_episode_out *out /* may be NULL */);
eg_plan_set *eg_plans_load(const char *path);
void eg_plans_free(eg_plan_set *);
/* Writes the plans as JSON Lines in the same schema, one object per line with its name: what eg_plans_load reads back.  The set is
 * validated first (eg_plans_validate). */
int32_t eg_plans_save(const eg_plan_set *, const char *path);

/* Plan edits: which actions of a plan matter?  eg_evaluate_plan_edits(ctx, policy, opts, base, edits, n_edits, seed,
 * first_episode_index, same_index, out) evaluates n_edits VARIANTS of one base plan (a plan set of exactly one plan), variant j being the
 * base with edit j applied to one year's list of one of its two lists:
 *   kind    EG_EDIT_NONE: the base plan itself (no other field is read), EG_EDIT_DELETE: entry `pos` removed, EG_EDIT_REPLACE: entry `pos`
 *           becomes `action`, EG_EDIT_INSERT: `action` inserted in front of entry `pos`
 *   list    0 = best_actions, 1 = best_deficit_actions
 *   year    the year index 0..25
 *   pos     a position in that year's list: 0..len-1 for delete and replace, 0..len for insert (len: append)
 *   action  replace and insert: a canonical index 0..60 (what eg_plans_validate accepts in either list)
 * Variant j is evaluated exactly as eg_evaluate_plans evaluates the edited plan as plan j — the same replay semantics, seeded draws when
 * a list runs out, no statistics, update or folds, the resident policy untouched, the batch left behind for eg_fetch / eg_fetch_record,
 * ranks of a group refused — at global episode first_episode_index + j (same_index = 0), or with same_index = 1 every variant at global
 * episode first_episode_index: all variants then see the same fallback draws and differ by their edit only.  The host uploads the base
 * plan's block once and 8 bytes per variant; the variants' plan blocks are written on the device (csrc/eg_plan_edits.h).
 * eg_plan_edits_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the edit and the field for a position out of range,
 * an insert that would make a list longer than 4 096 entries, an action >= 61, a year >= 26, an unknown kind or list, n_edits < 1, or a
 * base that is not exactly one valid plan. */
#define EG_EDIT_NONE 0
#define EG_EDIT_DELETE 1
#define EG_EDIT_REPLACE 2
#define EG_EDIT_INSERT 3
typedef struct { uint8_t kind, list; uint16_t year; uint32_t pos; uint8_t action; } eg_plan_edit;
int32_t eg_plan_edits_validate(const eg_plan_set *base, const eg_plan_edit *edits, int32_t n_edits);
int32_t eg_evaluate_plan_edits(eg_ctx *, const eg_policy_snapshot *policy, const eg_opts *, const eg_plan_set *base /* n_plans == 1 */,
                               const eg_plan_edit *edits, int32_t n_edits, uint64_t seed, uint64_t first_episode_index, int32_t same_index,
                               eg_episode_out *out /* may be NULL */);
/* Test hook: the plan block of plan / variant `plan` of the last plan or plan-edit batch as the replay kernels read it
 * (EG_PLAN_BLOCK_BYTES: per-year masks, prefix offsets, the two flat lists; csrc/eg_internal.h snap::kPlanStride), after the device has
 * finished that batch.  A plan-edit batch's blocks must equal, byte for byte, the blocks eg_evaluate_plans builds for the edited plans. */
#define EG_PLAN_BLOCK_BYTES 8832
int32_t eg_debug_fetch_plan_block(eg_ctx *, uint32_t plan, uint8_t *out /* EG_PLAN_BLOCK_BYTES */);

/* Greedy plan refinement: apply the best one-entry edit of a plan, again and again, without leaving the device.
 * eg_refine_plan(ctx, policy, opts, base, refine_opts, seed, episode_index, ...) starts from the base plan B_0 (a plan set of exactly one
 * plan).  In round r the VARIANTS of B_r are, in this order:
 *   1. the base itself (EG_EDIT_NONE); every best_actions entry deleted, in (year, position) order; every best_deficit_actions entry
 *      deleted likewise; every best_actions entry, in the same order, replaced by each action of replace_with in the given order — the
 *      order of the CLI's --sensitivity table;
 *   2. for every year 0..25 and each action of append_with in the given order, that action inserted behind the last entry of the
 *      year's best_actions list (an empty year: at position 0).  No appends while best_actions holds 4 096 entries.
 * All variants are evaluated as eg_evaluate_plan_edits(..., first_episode_index = episode_index, same_index = 1) evaluates them.
 * Variant j is a CANDIDATE when its status is EG_EP_OK and s_j = eg_rank_score(metrics_j, mode) is not NaN; the WINNER is the candidate
 * with the largest s_j, ties to the lowest j — variant 0 is the base, so only a strict improvement moves the plan.
 *   variant 0 is no candidate   stop with EG_REFINE_BASE_FAILED; B_r is returned, no step is recorded for the round
 *   the winner is variant 0     stop with EG_REFINE_LOCAL_OPTIMUM
 *   otherwise                   B_{r+1} is the winner's plan and a step is recorded: its edit (against B_r), its variant index, the round's
 *                               variant count, how many variants were no candidates, its score and metrics
 *   after max_rounds steps      stop with EG_REFINE_MAX_ROUNDS
 * The winner is picked on the device (csrc/eg_refine_many.h k_refine_pick_many) and its plan block becomes the next round's base there:
 * the call is eg_refine_plans' loop (below) over its one plan, which always has a launch to itself.  Per round the host uploads 16 bytes
 * per variant and 16 more and reads one entry of at most 128 bytes back.  The policy is checked, staged and uploaded once per call.  Everything else is the contract of eg_evaluate_plan_edits: no statistics, update or folds, the resident policy untouched, a
 * rank of a group refused; the last round's variants stay behind as the last batch for eg_fetch / eg_fetch_record.
 * *refined: the final plan (free with eg_plans_free); steps[max_rounds], *n_steps, *stop_reason; *start_score: s_0 of round 0 (NaN when
 * the base failed); `out` (one episode, may be NULL): the refined plan's record — variant 0 of the last round on LOCAL_OPTIMUM, the last
 * winner on MAX_ROUNDS, not written on BASE_FAILED.  A round that would enumerate more than EG_REFINE_MAX_VARIANTS variants is refused
 * (EG_ERR_BAD_ARG naming the round and the count): round 0 by eg_refine_validate, later rounds when they are reached.
 * eg_refine_validate runs the checks alone: mode 1 or 2, max_rounds >= 1, actions 0..60, no NULL list with a count, a base of exactly
 * one valid plan.
 * Under plan streams (eg_plan_streams_set, below) every round's variants run as R passes and the pick reads their committed metrics and status: no other change. */
#define EG_REFINE_LOCAL_OPTIMUM 0
#define EG_REFINE_MAX_ROUNDS 1
#define EG_REFINE_BASE_FAILED 2
#define EG_REFINE_MAX_VARIANTS 16384
typedef struct { int32_t mode /* 1 | 2 */, max_rounds; int32_t n_replace; const uint8_t *replace_with;
                 int32_t n_append; const uint8_t *append_with; } eg_refine_opts;
typedef struct { eg_plan_edit edit; int32_t variant, n_variants, n_failed; double score; double metrics[4]; } eg_refine_step;
int32_t eg_refine_validate(const eg_plan_set *base, const eg_refine_opts *);
int32_t eg_refine_plan(eg_ctx *, const eg_policy_snapshot *, const eg_opts *, const eg_plan_set *base /* 1 plan */,
                       const eg_refine_opts *, uint64_t seed, uint64_t episode_index,
                       eg_plan_set **refined /* eg_plans_free */, eg_refine_step *steps /* max_rounds */,
                       int32_t *n_steps, int32_t *stop_reason, double *start_score, eg_episode_out *out /* 1 episode or NULL */);

/* Many plans refined in one call: eg_refine_plans(ctx, policy, opts, bases, refine_opts, seed, episode_index, ...) takes a set of 1 ..
 * EG_REFINE_MAX_PLANS base plans (a whole Pareto front, the scenarios of --top-k) and refines every one of them as eg_refine_plan would.
 * For every plan p the following are EXACTLY what eg_refine_plan returns for a base set holding plan p alone, with the same policy, options,
 * refine_opts, seed and episode_index:
 *   *refined          plan p of the returned set (n_plans plans in the bases' order, their names kept; free with eg_plans_free)
 *   steps             row p of steps[n_plans][max_rounds], entries 0 .. n_steps[p]: every field — `variant`, `n_variants` and `n_failed`
 *                     count within the plan's own round, score and metrics bit for bit
 *   n_steps[p], stop_reason[p], start_score[p] (start_score may be NULL)
 *   out               row p of `out` (n_plans episodes, may be NULL): the refined plan's record — variant 0 of the plan's last round on
 *                     LOCAL_OPTIMUM, the last winner on MAX_ROUNDS; a row is NOT written when its plan stops with BASE_FAILED
 * (Of a record, n_chunks excepted: it counts what the search that really ran requested, and a launch of many plans' variants may run
 * the throughput kernels where a plan's own round would run the small-batch kernel.)
 * Plans are independent: they stop in different rounds and for different reasons, and a stopped plan takes no further part.  What makes
 * the call worth having is that the rounds are stepped TOGETHER: per round the still-active plans, in ascending order, are packed into
 * launches of at most EG_REFINE_MAX_VARIANTS variants, a SEGMENT of consecutive variants per plan (a plan never straddles two launches);
 * csrc/eg_refine_many.h k_plan_edits_many writes every variant's block from its plan's base block, the plan batch runs over the whole
 * launch with same_index = 1 — a variant's result does not depend on what else is in its launch —, and k_refine_pick_many picks a winner
 * per segment and makes its block that plan's next base.  Per launch the host uploads 16 bytes per variant and 16 per segment and reads
 * one entry of at most 128 bytes per segment back, in ONE copy: the launch's only synchronisation.  The base blocks of all plans go up
 * once.  The result does not depend on how the library packs plans into launches.  The environment variable
 * EIRGRID_REFINE_LAUNCH_VARIANTS (read at every call, clamped to 1..16 384) lowers the variants a launch may hold — a plan with more gets
 * a launch to itself —, for tests that want many launches per round at small sizes.
 * A later round of some plan that would enumerate more than EG_REFINE_MAX_VARIANTS variants fails the WHOLE call with EG_ERR_BAD_ARG, the
 * message naming the plan and the round; nothing is returned then.
 * Everything else is eg_refine_plan's contract: no statistics, update or folds, the resident policy untouched, a rank of a group refused,
 * the policy checked, staged and uploaded once per call; what stays behind as the last batch for eg_fetch / eg_fetch_record is the LAST
 * launch's variants.
 * eg_refine_plans_validate runs the checks alone and names the plan in every message about one ("plan 3: round 0 enumerates ..."): a
 * valid set (eg_plans_validate) of 1..EG_REFINE_MAX_PLANS plans; the option checks of eg_refine_validate; per plan, the variant count of
 * round 0.
 * Under plan streams (eg_plan_streams_set, below) every launch runs as R passes and every plan's pick reads committed metrics and status (eg_refine_plans_moves alike): no other change. */
#define EG_REFINE_MAX_PLANS 256          /* = EG_PARETO_MAX: a whole front fits */
int32_t eg_refine_plans_validate(const eg_plan_set *bases, const eg_refine_opts *);
int32_t eg_refine_plans(eg_ctx *, const eg_policy_snapshot *, const eg_opts *, const eg_plan_set *bases /* 1..EG_REFINE_MAX_PLANS */,
                        const eg_refine_opts *, uint64_t seed, uint64_t episode_index,
                        eg_plan_set **refined      /* n_plans plans in the bases' order, names kept; eg_plans_free */,
                        eg_refine_step *steps      /* [n_plans][max_rounds], row p = plan p */,
                        int32_t *n_steps           /* [n_plans] */, int32_t *stop_reason /* [n_plans] */,
                        double *start_score        /* [n_plans] or NULL */, eg_episode_out *out /* n_plans episodes or NULL */);

/* Plan moves: should this plant be built in another year?  A MOVE takes one entry of one year's list out and puts it back into another
 * year's list (or elsewhere in the same one); both lists keep their lengths.  As two edits it is a delete and then an insert, which the
 * greedy refinement cannot cross when the first half alone is worse than the base; as a move it is one variant.
 * eg_evaluate_plan_moves evaluates n_moves VARIANTS of one base plan (a plan set of exactly one plan), variant j being the base with
 * move j applied to one of its two lists:
 *   list     0 = best_actions, 1 = best_deficit_actions
 *   year     the year index 0..25 the entry is taken from, and `pos` its position there, 0..len-1
 *   to_year  the year index 0..25 it goes to (to_year == year: a reorder within the year)
 *   to_pos   it is put back in front of entry to_pos of year to_year's list AS THAT LIST STANDS AFTER THE REMOVAL: 0..len', len' being
 *            the length of year to_year, minus one when to_year == year; to_pos == len' puts it behind the last entry
 * to_year == year with to_pos == pos is the base plan itself, the "none" of moves, so variant 0 of a batch can be the base.
 * Everything else is the contract of eg_evaluate_plan_edits, word for word: variant j is evaluated exactly as eg_evaluate_plans
 * evaluates the moved plan as plan j — the same replay semantics, seeded draws when a list runs out, no statistics, update or folds, the
 * resident policy untouched, the batch left behind for eg_fetch / eg_fetch_record / eg_debug_fetch_plan_block, ranks of a group refused —
 * at global episode first_episode_index + j (same_index = 0), or with same_index = 1 every variant at first_episode_index.  The host
 * uploads the base plan's block once and 8 bytes per variant; the variants' plan blocks are written on the device
 * (csrc/eg_plan_moves.h k_plan_moves).  The list lengths do not change, so every variant takes the base's short or long replay route.
 * eg_plan_moves_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the move and the field ("move 2: to_pos 4 outside
 * best_actions year 2031 (3 entries after the removal)") for a list above 1, a year or to_year >= 26, a pos outside the year's list, a
 * to_pos outside 0..len', n_moves < 1, NULL moves, or a base that is not exactly one valid plan. */
typedef struct { uint8_t list, to_year; uint16_t year; uint32_t pos, to_pos; } eg_plan_move;   /* 12 bytes */
int32_t eg_plan_moves_validate(const eg_plan_set *base /* 1 plan */, const eg_plan_move *moves, int32_t n_moves);
int32_t eg_evaluate_plan_moves(eg_ctx *, const eg_policy_snapshot *policy, const eg_opts *, const eg_plan_set *base /* n_plans == 1 */,
                               const eg_plan_move *moves, int32_t n_moves, uint64_t seed, uint64_t first_episode_index, int32_t same_index,
                               eg_episode_out *out /* may be NULL */);

/* Refinement with moves: eg_refine_plans_moves is eg_refine_plans with one more family of variants at the END of a round's enumeration.
 * After the variants of eg_refine_plans (the base, the deletes, the replaces, the appends) come the MOVE variants: for every
 * best_actions entry in (year, position) order, and for each shift d in the order -1, +1, -2, +2, ..., -max_shift, +max_shift with
 * 0 <= year + d <= 25, that entry moved behind the last entry of year year + d (eg_plan_move: list 0, to_year = year + d, to_pos = the
 * length of that year's list).  Entries of best_deficit_actions are not moved.  Variant 0 stays the base and ties go to the lowest
 * variant, so on a tie a plain edit wins over a move.
 * A step says with is_move which of `edit` / `move` it holds (against the plan of its round); the other one is zeroed.
 * EG_REFINE_MAX_VARIANTS holds over edits and moves together, with eg_refine_plans' messages: round 0 is refused by the validator, a
 * later round fails the whole call.  The move variants ride in the launches of eg_refine_plans, behind their plan's edits in its
 * segment: a move is packed into 8 bytes whose first byte is no edit kind, k_plan_edits_many writes a copy of the base for it,
 * csrc/eg_plan_moves.h k_plan_moves overwrites that block behind it on the same stream, and k_refine_pick_many picks as before.
 * With max_shift == 0 every returned field equals eg_refine_plans' and is_move is 0 throughout.  Everything else is eg_refine_plans'
 * contract.
 * eg_refine_plans_moves_validate runs the checks alone: those of eg_refine_plans_validate, move options that are not NULL, max_shift
 * 0..25, and per plan the variant count of round 0, moves included. */
typedef struct { int32_t max_shift; } eg_refine_move_opts;   /* 0..25 years; 0: no moves */
typedef struct { int32_t is_move; eg_plan_edit edit; eg_plan_move move; int32_t variant, n_variants, n_failed;
                 double score; double metrics[4]; } eg_refine_move_step;
int32_t eg_refine_plans_moves_validate(const eg_plan_set *bases, const eg_refine_opts *, const eg_refine_move_opts *);
int32_t eg_refine_plans_moves(eg_ctx *, const eg_policy_snapshot *, const eg_opts *, const eg_plan_set *bases /* 1..EG_REFINE_MAX_PLANS */,
                              const eg_refine_opts *, const eg_refine_move_opts *, uint64_t seed, uint64_t episode_index,
                              eg_plan_set **refined, eg_refine_move_step *steps /* [n_plans][max_rounds] */, int32_t *n_steps,
                              int32_t *stop_reason, double *start_score, eg_episode_out *out);

/* Plan crosses: what does A's first decade followed by B's last fifteen years score?  A CROSS splices the years of one plan into another:
 * the first variant with two parents.  eg_evaluate_plan_crosses evaluates n_crosses VARIANTS over a set of 1..EG_CROSS_MAX_PARENTS parent
 * plans, variant j being parent `a` with BOTH lists (best_actions and best_deficit_actions) of the years from_year <= y < to_year
 * replaced by parent `b`'s lists of those years:
 *   a, b                 indices into the parent set, 0..n_plans-1
 *   from_year, to_year   year indices with 0 <= from_year <= to_year <= 26; the window is [from_year, to_year)
 * from_year == to_year or a == b is parent `a` itself, the "none" of crosses, so the parents can ride in the batch; to_year == 26 is the
 * one-point crossover (head of a, tail of b); to_year == from_year + 1 transplants one year.
 * Everything else is the contract of eg_evaluate_plan_edits, word for word: variant j is evaluated exactly as eg_evaluate_plans
 * evaluates the host-built child as plan j — the same replay semantics, seeded draws when a list runs out, no statistics, update or folds,
 * the resident policy untouched, the batch left behind for eg_fetch / eg_fetch_record / eg_debug_fetch_plan_block, ranks of a group
 * refused — at global episode first_episode_index + j (same_index = 0), or with same_index = 1 every variant at first_episode_index.  The
 * host uploads every parent's block once and 8 bytes per variant; the variants' plan blocks are written on the device
 * (csrc/eg_plan_crosses.h k_plan_crosses).  A child's best_actions length differs from its parents', so the short or long replay route
 * is chosen per variant from the counts, as eg_evaluate_plans chooses it.
 * eg_plan_crosses_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the cross and the field ("cross 7: best_actions
 * would hold 4212 entries (at most 4096)") for a parent set that is not a valid set of 1..EG_CROSS_MAX_PARENTS plans, n_crosses outside
 * 1..EG_CROSS_MAX_VARIANTS, NULL crosses, a or b >= n_plans, to_year > 26, from_year > to_year, or a child whose best_actions or
 * best_deficit_actions would exceed 4 096 entries.  Nothing is launched after a refusal.
 * Under plan streams (eg_plan_streams_set, below) the batch runs as R passes and comes back with committed metrics and status (eg_evaluate_plans, _plan_edits, _plan_moves, _plan_rewrites alike): no other change. */
#define EG_CROSS_MAX_PARENTS 256      /* = EG_PARETO_MAX */
#define EG_CROSS_MAX_VARIANTS 16384   /* = EG_REFINE_MAX_VARIANTS */
typedef struct { uint16_t a, b; uint8_t from_year, to_year; } eg_plan_cross;   /* 6 bytes */
int32_t eg_plan_crosses_validate(const eg_plan_set *parents, const eg_plan_cross *crosses, int32_t n_crosses);
int32_t eg_evaluate_plan_crosses(eg_ctx *, const eg_policy_snapshot *policy, const eg_opts *, const eg_plan_set *parents,
                                 const eg_plan_cross *crosses, int32_t n_crosses, uint64_t seed, uint64_t first_episode_index,
                                 int32_t same_index, eg_episode_out *out /* may be NULL */);

/* Plan rewrites: what is a technology worth to this plan?  What does it score without nuclear, with offshore wind built as onshore, with
 * every plant bought at the 100 % cost tier, with nothing built after 2040?  All of these are one operation: an ACTION MAP — 61 entries,
 * to[e] being the action that entry e becomes, or EG_REWRITE_DROP: e is taken out — applied to every entry of a window of years of a plan.
 * eg_evaluate_plan_rewrites evaluates n_rewrites VARIANTS over a set of 1..EG_CROSS_MAX_PARENTS plans and n_maps maps, variant j being plan
 * `plan` of the set changed as follows:
 *   lists                bit 0: best_actions changes, bit 1: best_deficit_actions changes; a list whose bit is clear is the plan's own
 *   from_year, to_year   year indices with 0 <= from_year <= to_year <= 26; only the years of the window [from_year, to_year) change
 *   map                  an index into `maps`; in the years of the window a selected list becomes [m.to[e] for e in list if m.to[e] !=
 *                        EG_REWRITE_DROP], the order of the kept entries preserved
 * lists == 0, from_year == to_year, or a map that is the identity on the entries it meets give the plan itself, the "none" of rewrites,
 * so the plans can ride in the batch.  A rewrite never lengthens a list, so no variant can exceed 4 096 entries.
 * THE DEFICIT LIST IS NOT THE PLAN LIST.  A dropped best_actions entry is simply not acted on: a year's action count is the length of
 * its list.  A best_deficit_actions list that has become too short is REFILLED, by seeded draws from the fixed fallback distribution
 * (sampling.rs:492-528), and that distribution holds gas peakers.  So a technology is taken out of the deficit list by SUBSTITUTING it,
 * not by dropping it.
 * Everything else is the contract of eg_evaluate_plan_crosses, word for word: variant j is evaluated exactly as eg_evaluate_plans
 * evaluates the host-built child as plan j — the same replay semantics, seeded draws when a list runs out, no statistics, update or folds,
 * the resident policy and the context's archives untouched, the batch left behind for eg_fetch / eg_fetch_record /
 * eg_debug_fetch_plan_block, ranks of a group refused — at global episode first_episode_index + j (same_index = 0), or with same_index = 1
 * every variant at first_episode_index.  The host uploads every plan's block once, the maps once (64 bytes each) and 8 bytes per variant;
 * the variants' plan blocks are written on the device (csrc/eg_plan_rewrites.h k_plan_rewrites).  The short or long replay route is
 * chosen per variant from the child's best_actions length: a rewrite can make a long plan short.
 * eg_plan_rewrites_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the rewrite or the map and the field ("map 3:
 * to[17] = 200 (0..60 or 0xFF drop)", "rewrite 5: plan 4 >= n_plans 4") for a set that is not a valid set of 1..EG_CROSS_MAX_PARENTS
 * plans, n_maps outside 1..EG_REWRITE_MAX_MAPS, NULL maps, a map entry in 61..254, n_rewrites outside 1..EG_REWRITE_MAX_VARIANTS, NULL
 * rewrites, plan >= n_plans, map >= n_maps, to_year > 26, from_year > to_year, lists > 3, or pad != 0.  Nothing is launched after a
 * refusal, and the previous last batch stays fetchable. */
#define EG_REWRITE_DROP 0xFF
#define EG_REWRITE_MAX_MAPS 256
#define EG_REWRITE_MAX_VARIANTS 16384          /* = EG_CROSS_MAX_VARIANTS */
typedef struct { uint8_t to[EG_N_ACTIONS]; } eg_action_map;                                   /* 61 bytes */
typedef struct { uint16_t plan, map; uint8_t from_year, to_year, lists, pad; } eg_plan_rewrite; /* 8 bytes */
int32_t eg_plan_rewrites_validate(const eg_plan_set *plans, const eg_action_map *maps, int32_t n_maps,
                                  const eg_plan_rewrite *rewrites, int32_t n_rewrites);
int32_t eg_evaluate_plan_rewrites(eg_ctx *, const eg_policy_snapshot *, const eg_opts *, const eg_plan_set *plans /* 1..EG_CROSS_MAX_PARENTS */,
                                  const eg_action_map *maps, int32_t n_maps, const eg_plan_rewrite *rewrites, int32_t n_rewrites,
                                  uint64_t seed, uint64_t first_episode_index, int32_t same_index, eg_episode_out *out /* may be NULL */);

/* Plan constraints: bounds on the yearly rows of a plan batch's records, enforced on the device.  The plan searches judge a variant by its
 * four end-of-run metrics; "net zero from 2040 on", "no year's total cost above a budget", "the balance never below a reserve",
 * "cumulative emissions under a carbon budget" are statements about the 26 x 21 yearly rows every record carries (EG_Y_*).  A context
 * holds up to EG_CONSTRAINTS_MAX constraints; behind the rollout grids of every plan batch one kernel (csrc/eg_plan_constraints.h
 * k_plan_constraints) judges them over the batch's records and DEMOTES the status of a variant that violates one to EG_EP_INFEASIBLE.
 * Every search already skips a variant whose status is not EG_EP_OK, so every search becomes a constrained search.
 * THE DEFINITION.  For one record with rows v[y][col] (y = 0..25) the EXCESS of a constraint {column, aggregate, op, from_year, to_year,
 * bound} — the window is the years from_year <= y < to_year — is
 *   EG_AGG_EVERY   x_y = v[y][column] - bound for EG_OP_LE, bound - v[y][column] for EG_OP_GE (one rounding).  e = x_from; then for
 *                  y = from_year + 1 .. to_year - 1 in order: if e is NaN it stays, else if x_y is NaN or x_y > e then e = x_y.  The
 *                  excess is e: the largest x_y, the first of equal ones (-0.0 and +0.0 are equal), and NaN once any x_y is NaN.
 *   EG_AGG_SUM     s = v[from_year][column], then s = s + v[y][column] for y = from_year + 1 .. to_year - 1 in order (one rounding each,
 *                  no fused multiply-add).  The excess is s - bound for EG_OP_LE and bound - s for EG_OP_GE.
 * A NaN excess is reported as the canonical quiet NaN (bits 0x7FF8000000000000), whatever payload or sign the arithmetic gave it.  The
 * constraint is SATISFIED iff excess <= 0; NaN violates.  A negative excess is the slack.  This literal order is the definition.
 * AFTER A PLAN BATCH with k > 0 constraints set, for variant j of the batch:
 *   status EG_EP_OK on entry     excess[j][0..k) as above; violated[j] has bit i set iff constraint i is violated; the status becomes
 *                                EG_EP_INFEASIBLE iff violated[j] != 0.  The metrics and every other byte of the record are untouched.
 *   any other status on entry    the status is untouched, violated[j] = 0 and the excess row is all (canonical) NaN.
 * eg_plan_constraints_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the constraint's index and the field
 * ("constraint 3: column 21 (an EG_Y_* column 0..20)") for n outside 0..EG_CONSTRAINTS_MAX, NULL constraints with n > 0, column > 20, an
 * unknown aggregate or op, from_year >= to_year, to_year > 26 or a bound that is not finite.  eg_plan_constraints_set validates, then
 * uploads the constraints (16 bytes each) to a device buffer of the context; n = 0 clears them.  A rank of a group is refused.  They hold
 * for every later plan batch of the context — eg_evaluate_plans, _plan_edits, _plan_moves, _plan_crosses, _plan_rewrites,
 * eg_refine_plan, eg_refine_plans, eg_refine_plans_moves, eg_breed_plans, eg_explore_plans: one launch at the end of every batch of
 * variants these launch, on the stream the batch ran on, so the picks and folds enqueued behind it read the demoted statuses.  While
 * constraints are set these calls refuse eg_opts.write_yearly = 0: the rows are what is judged.  Training batches (eg_rollout_batch,
 * eg_rollout_launch, eg_train_step, eg_device_rollout, eg_device_step, groups) are never judged, and neither are their best_result,
 * top-K and Pareto folds.  What follows for the searches: a refinement whose base is infeasible stops with EG_REFINE_BASE_FAILED; a
 * step's n_failed counts the infeasible variants with the failed ones; eg_explore_plans from infeasible starts admits their feasible
 * neighbours (the way to repair a plan), eg_breed_plans from infeasible parents keeps their feasible children only.
 * eg_fetch_plan_feasibility serves the LAST batch (for a search: the last launch of the call): violated[n] and excess[n][k], n =
 * eg_last_batch_size(), k the constraints that were set WHEN IT RAN — not those set now: setting or clearing constraints afterwards
 * changes neither k nor what is served; either pointer may be NULL.  EG_ERR_BAD_ARG when the last batch ran without constraints (a
 * training batch, a plan batch with none set, no batch at all).  eg_last_batch_constraints returns that k (0 when the last batch was
 * not judged; EG_ERR_BAD_ARG for a NULL context) and copies the k constraints the batch was judged under into `out` unless it is NULL: a
 * caller sizes the excess buffer from it.
 * One parser for every front end: eg_plan_constraint_parse reads "[sum(]COLUMN[)] (<=|>=) BOUND [@FROM[:TO]]" — COLUMN a lower-case EG_Y_*
 * name (year, pop, usage, gen, balance, opinion, yearly_capital, total_capital, inflation, co2, offset, net_co2, yearly_credit,
 * total_credit, yearly_sales, total_sales, active_gens, upgrade_costs, closure_costs, yearly_total_cost, total_cost), BOUND a finite
 * number, FROM and TO calendar years 2025..2050, both inclusive; no @ means all 26 years, @FROM alone means FROM..2050 ("net_co2 <= 0
 * @2040", "sum(net_co2) <= 4e8", "balance >= 500 @2030:2039").  EG_ERR_BAD_ARG with a message that quotes the offending token.
 * eg_plan_constraint_format writes the same form (the bound with 17 significant digits, so parse(format(c)) == c) into buf; EG_ERR_BAD_ARG
 * for a constraint eg_plan_constraints_validate refuses or a buffer that is too small (EG_CONSTRAINT_SPEC_MAX bytes always suffice).
 * Test hooks (they refuse a rank of a group): eg_debug_load_yearly overwrites the yearly rows of the n records eg_debug_load_batch made
 * (n = eg_last_batch_size()); eg_debug_constrain_last_batch launches k_plan_constraints (with a build constraint set: k_build_constraints,
 * below) over the last batch through the launcher a plan batch uses (EG_ERR_BAD_ARG with no constraints set or no last batch). */
#define EG_CONSTRAINTS_MAX 32
#define EG_AGG_EVERY 0   /* each year of the window */
#define EG_AGG_SUM 1     /* the window's sum */
#define EG_OP_LE 0
#define EG_OP_GE 1
#define EG_CONSTRAINT_SPEC_MAX 96
typedef struct { uint8_t column /* EG_Y_*, 0..20 */, aggregate, op, from_year, to_year /* 0 <= from < to <= 26 */, pad[3]; double bound /* finite */; } eg_plan_constraint; /* 16 bytes */
int32_t eg_plan_constraints_validate(const eg_plan_constraint *constraints, int32_t n);
int32_t eg_plan_constraints_set(eg_ctx *, const eg_plan_constraint *constraints, int32_t n /* 0: clear */);
int32_t eg_fetch_plan_feasibility(eg_ctx *, uint32_t *violated /* [n] or NULL */, double *excess /* [n][k_rows + k_builds] or NULL */);
int32_t eg_last_batch_constraints(const eg_ctx *, eg_plan_constraint *out /* [EG_CONSTRAINTS_MAX] or NULL */);
int32_t eg_plan_constraint_parse(const char *spec, eg_plan_constraint *out);
int32_t eg_plan_constraint_format(const eg_plan_constraint *c, char *buf, int32_t len);
int32_t eg_debug_load_yearly(eg_ctx *, const double *yearly /* [n][26][21] */, uint32_t n);
int32_t eg_debug_constrain_last_batch(eg_ctx *);

/* Build constraints: bounds on what a plan BUILDS, judged on the device with the plan constraints above.  The yearly rows hold totals
 * (gen, co2, active_gens), no technology: "no new gas", "at most two nuclear plants", "no more than four onshore wind farms a year", "at
 * least as many batteries as wind farms by 2035", "at most ten carbon-credit purchases" are statements about the fleet an episode
 * actually built — gen_pack[n_gens] and off_pack[n_offsets] of its record, which include the repair loop's and the fallback draws' builds
 * (dropping a technology from a plan's text does not keep a fallback draw from building it) and the entries a replay applies twice.
 * THE DEFINITION.  There are EG_BUILD_CLASSES classes: 0..14 the generator types in models/generator.rs order, 15..18 Forest, Wetland,
 * ActiveCapture, CarbonCredit.  For one record, c[y][q] (y = 0..25) counts the list entries that match: of gen_pack, the entries
 * i < clamp(n_gens, 0, EG_MAX_GENS) with (pk & 15) == q, q < 15, and ((pk >> 4) & 31) == y; of off_pack, the entries
 * i < clamp(n_offsets, 0, EG_MAX_OFFSETS) with (pk & 15) < 4, q == 15 + (pk & 15), and ((pk >> 4) & 31) == y.  An entry whose class is out
 * of range (generator type 15, offset type >= 4) or whose year index is >= 26 counts nowhere; what lies at or behind the counts is never
 * read as data.  The VALUE of a count vector m[0..19) under a constraint's weights is
 *   s = +0.0; for q = 0..18 in order: s = s + weight[q] * (double)m[q]      (the product rounded once, the sum rounded once, no FMA)
 * and the EXCESS of a constraint {aggregate, op, from_year, to_year, bound, weight[19]} over the window from_year <= y < to_year is
 *   EG_AGG_EVERY   x_y = value(c[y]) - bound for EG_OP_LE, bound - value(c[y]) for EG_OP_GE, folded over the window exactly as the row
 *                  definition folds it: e = x_from, then if e is NaN it stays, else if x_y is NaN or x_y > e then e = x_y (the largest,
 *                  the first of equal ones).  A build-rate cap per year.
 *   EG_AGG_SUM     m[q] = the sum of c[y][q] over the window (integer, exact); the excess is value(m) - bound or bound - value(m).  A
 *                  total over the window.
 * SATISFIED iff excess <= 0.  The weight cap keeps every value finite, so no NaN arises; a NaN excess would be stored as the canonical
 * quiet NaN all the same, so the two kinds share one rule.
 * HOW THE TWO KINDS LIVE TOGETHER.  A context holds row constraints (eg_plan_constraints_set) and build constraints
 * (eg_build_constraints_set), together at most EG_CONSTRAINTS_MAX: either setter refuses a count that would take the total above it,
 * naming both counts; n = 0 clears that kind only.  A judged batch has k = k_rows + k_builds constraints; mask bit i and excess column i
 * number the row constraints first, then the build constraints.  With a build constraint set, csrc/eg_build_constraints.h
 * k_build_constraints runs in place of k_plan_constraints behind every plan batch and judges both kinds in one pass — one mask, one
 * excess row, one demotion a record; with none set nothing differs from the section above.  eg_fetch_plan_feasibility then serves
 * excess[n][k_rows + k_builds]; eg_last_batch_constraints keeps returning the ROW constraints and k_rows, eg_last_batch_build_constraints
 * returns k_builds (0 when the last batch was not judged) and copies the build constraints it was judged under unless `out` is NULL;
 * eg_repair_plans and eg_debug_repair_pick_many take k = k_rows + k_builds weights and refuse only when neither kind is set;
 * eg_debug_constrain_last_batch runs when either kind is set.  The write_yearly = 0 refusal stays tied to row constraints: build
 * constraints alone do not read the rows.  Groups and training batches are not judged, as above.
 * eg_build_constraints_validate: EG_ERR_BAD_ARG naming index and field ("constraint 3: weight[7] nan (finite, at most 1e300 in
 * magnitude)") for n outside 0..EG_CONSTRAINTS_MAX, NULL with n > 0, an unknown aggregate or op, to_year > 26, from_year >= to_year, a
 * bound that is not finite, a weight that is not finite or above 1e300 in magnitude, weights that are all zero.
 * TEXT FORM, one parser and one formatter: "[sum(]built(TERMS)[)] (<=|>=) BOUND [@FROM[:TO]]", TERMS = [W*]CLASS {(+|-) [W*]CLASS}, CLASS a
 * generator type name (OnshoreWind, OffshoreWind, DomesticSolar, CommercialSolar, UtilitySolar, Nuclear, CoalPlant, GasCombinedCycle,
 * GasPeaker, Biomass, HydroDam, PumpedStorage, BatteryStorage, TidalGenerator, WaveEnergy), an offset name (Forest, Wetland,
 * ActiveCapture, CarbonCredit) or `any` (all 15 generator types); W a finite number, 1 when absent; a class named twice is refused; the
 * window as in the row grammar ("built(GasPeaker + GasCombinedCycle) <= 0", "sum(built(Nuclear)) <= 2", "built(OnshoreWind) <= 4
 * @2025:2034", "sum(built(BatteryStorage - OnshoreWind)) >= 0 @2025:2035", "sum(built(CarbonCredit)) <= 10").  Errors quote the offending
 * token.  eg_build_constraint_format writes the classes with a weight other than zero in index order, the bound and every weight other
 * than 1 with 17 significant digits, `any` when weights 0..14 are equal and not zero and 15..18 are zero, so parse(format(c)) == c (a
 * weight of -0.0 reads back as +0.0); EG_BUILD_SPEC_MAX bytes always suffice.
 * Test hook (it refuses a rank of a group): eg_debug_load_built overwrites the two counts and the two lists of the n records
 * eg_debug_load_batch made (n = eg_last_batch_size()); whole rows are copied, what lies behind the counts included. */
#define EG_BUILD_CLASSES 19   /* 0..14: the generator types in models/generator.rs order (gen_pack & 15);
                                 15..18: Forest, Wetland, ActiveCapture, CarbonCredit (15 + (off_pack & 15)) */
#define EG_BUILD_SPEC_MAX 1024
typedef struct { uint8_t aggregate, op, from_year, to_year /* 0 <= from < to <= 26 */, pad[4]; double bound /* finite */;
                 double weight[EG_BUILD_CLASSES] /* each finite, |w| <= 1e300, not all zero */; } eg_build_constraint; /* 168 bytes */
int32_t eg_build_constraints_validate(const eg_build_constraint *constraints, int32_t n);
int32_t eg_build_constraints_set(eg_ctx *, const eg_build_constraint *constraints, int32_t n /* 0: clear */);
int32_t eg_last_batch_build_constraints(const eg_ctx *, eg_build_constraint *out /* [EG_CONSTRAINTS_MAX] or NULL */);
int32_t eg_build_constraint_parse(const char *spec, eg_build_constraint *out);
int32_t eg_build_constraint_format(const eg_build_constraint *c, char *buf, int32_t len);
int32_t eg_debug_load_built(eg_ctx *, const int32_t *n_gens /* [n] */, const uint16_t *gen_pack /* [n][EG_MAX_GENS] */,
                            const int32_t *n_offsets /* [n] */, const uint16_t *off_pack /* [n][EG_MAX_OFFSETS] */, uint32_t n);

/* Plan repair: what is the smallest change that makes this plan legal?  eg_repair_plans is a greedy descent on the violation of the
 * context's plan constraints, for the plans eg_refine_plans stops on with EG_REFINE_BASE_FAILED: per round, of a plan's one-entry
 * variants, it takes the one that violates least.
 * THE VIOLATION MEASURE.  A variant j of a batch judged under k constraints, with weights w[0..k) — each finite and > 0; NULL: every
 * weight 1.0 — has
 *   V_j = t_0 + t_1 + ... + t_{k-1}, folded from +0.0 in constraint order, one rounding per addition, no fused multiply-add
 *   t_i = +inf               if excess[j][i] is NaN
 *         w_i * excess[j][i]  if excess[j][i] > 0 (one rounding)
 *         +0.0               otherwise
 * V_j == 0 exactly when violated[j] == 0 (a product that underflows to zero aside: the rounds go by V).  A record whose status is
 * neither EG_EP_OK nor EG_EP_INFEASIBLE has no V.
 * A ROUND.  The variants of the plan B_r are those of eg_refine_plans_moves for the same eg_refine_opts / eg_refine_move_opts — the
 * move options may be NULL: no moves —, in its enumeration and order, evaluated the same way under the context's constraints.  Variant
 * j is a CANDIDATE when its status is EG_EP_OK or EG_EP_INFEASIBLE and s_j = eg_rank_score(metrics_j, mode) is not NaN.  Variant 0 is
 * the base.
 *   variant 0 is no candidate   stop with EG_REPAIR_BASE_FAILED; B_r is returned, no step is recorded for the round
 *   V_0 == 0                    stop with EG_REPAIR_FEASIBLE (only round 0 can end this way)
 *   otherwise                   the WINNER is the candidate with V_j < V_0 strictly and the smallest V_j, ties to the largest s_j, then to
 *                               the lowest j (inf < inf is false: a base at +inf moves only to a finite V)
 *   there is no such candidate  stop with EG_REPAIR_STUCK
 *   there is one                B_{r+1} is the winner's plan and a step is recorded: its edit or move (against B_r), its variant index,
 *                               the round's variant count, how many variants were no candidates and how many candidates had V == 0, its
 *                               mask, V, score and metrics.  A winner with V == 0 stops with EG_REPAIR_FEASIBLE at once — this is
 *                               checked first —, otherwise max_rounds steps stop with EG_REPAIR_MAX_ROUNDS
 * V falls strictly from step to step, so the descent cannot cycle.
 * The call is eg_refine_plans_moves' loop with another pick: the same packing of plans into launches (EIRGRID_REFINE_LAUNCH_VARIANTS),
 * the same kernels in front of the rollout grids, k_plan_constraints behind them, then csrc/eg_repair.h k_repair_pick_many, a workgroup
 * per plan of the launch, which folds V from the excess rows, picks and makes the winner's block the plan's next base.  The weights go
 * up with the launch's other inputs; one entry of at most 128 bytes per plan comes back, in the launch's one copy.  Per plan the result
 * equals the call over that plan alone; it does not depend on how plans are packed into launches (a record's n_chunks aside, as for
 * eg_refine_plans).
 *   *repaired          the plans as the descent left them, in the bases' order, names kept (free with eg_plans_free)
 *   steps              [n_plans][max_rounds], row p = plan p, entries 0 .. n_steps[p]
 *   stop_reason[p], start_violation[p] (V_0 of round 0; NaN when the base failed), final_violation[p] (V of the returned plan; NaN when
 *                      the base failed in round 0); either violation pointer may be NULL
 *   out                row p (n_plans episodes, may be NULL): the last winner's record when the plan stops on a step; variant 0's of the
 *                      last round for a feasible base and on EG_REPAIR_STUCK; not written on EG_REPAIR_BASE_FAILED
 * k is the number of constraints set on the context.  EG_ERR_BAD_ARG, the message naming the cause: no constraints set, a weight that is
 * not finite or not > 0, a rank of a group, whatever eg_refine_plans_moves_validate refuses (with NULL move options: what
 * eg_refine_plans_validate refuses).  Everything else is eg_refine_plans' contract: no statistics, update or folds, the resident policy,
 * the context's constraints and its Pareto archive untouched; the last launch's variants stay behind as the last batch.
 * eg_repair_plans_validate runs the checks alone, for k constraints. */
#define EG_REPAIR_FEASIBLE 0
#define EG_REPAIR_MAX_ROUNDS 1
#define EG_REPAIR_BASE_FAILED 2
#define EG_REPAIR_STUCK 3
typedef struct { int32_t is_move; eg_plan_edit edit; eg_plan_move move; int32_t variant, n_variants, n_failed, n_feasible;
                 uint32_t violated; double violation, score, metrics[4]; } eg_repair_step;
int32_t eg_repair_plans_validate(const eg_plan_set *bases, const eg_refine_opts *, const eg_refine_move_opts * /* or NULL */,
                                 const double *weights /* [k] or NULL */, int32_t k /* 1..EG_CONSTRAINTS_MAX */);
int32_t eg_repair_plans(eg_ctx *, const eg_policy_snapshot *, const eg_opts *, const eg_plan_set *bases /* 1..EG_REFINE_MAX_PLANS */,
                        const eg_refine_opts *, const eg_refine_move_opts * /* or NULL */, const double *weights /* [k] or NULL */,
                        uint64_t seed, uint64_t episode_index, eg_plan_set **repaired, eg_repair_step *steps /* [n_plans][max_rounds] */,
                        int32_t *n_steps, int32_t *stop_reason, double *start_violation, double *final_violation, eg_episode_out *out);

/* Plan streams: every plan batch judged over R draw streams, on the device.  A plan batch runs each variant once, at seed + first_index:
 * a replay reads no seeded draw only while its two lists last, and where best_deficit_actions runs short the repair loop falls back to
 * sampled draws — so a variant the searches made by deleting, splicing or dropping entries is judged by one stream's luck.  With
 * R = n_streams >= 2 set on a context, every later plan batch of it (everything that launches a plan batch: eg_evaluate_plans, _plan_edits,
 * _plan_moves, _plan_crosses, _plan_rewrites, eg_refine_plan, eg_refine_plans, eg_refine_plans_moves, eg_breed_plans, eg_explore_plans)
 * runs R PASSES.  Pass r is the batch exactly as it runs without streams at first_index + r: the same routing, the same long-plan chunks,
 * the constraint kernel behind the grids when constraints are set.  The passes run from r = R - 1 down to r = 0, so when the batch
 * returns the records hold STREAM 0's EPISODE — rows, lists, gen_pack, and the feasibility masks and excess rows
 * eg_fetch_plan_feasibility serves are what the batch holds without streams — but for metrics[4] and status, which hold the COMMITTED
 * outcome below (the records are not cleared between passes any more than between batches: what lies behind a list's count is whatever
 * was written there last).  eg_last_batch_size and the first index of the batch are as after one pass at first_index.  Behind each pass
 * csrc/eg_ensemble.h k_ensemble_keep copies metrics and status of the n records into slab r of a store of the context (40 bytes a variant
 * and stream, reserved at the first batch that needs it); behind the last pass k_ensemble_commit runs once, a wave a variant and a lane a
 * stream, overwrites every record's metrics and status and writes an eg_ensemble_row.  The picks and folds a search enqueues behind a
 * batch, and eg_pareto_fold_last_batch, read the committed outcome: every search becomes a search on committed outcomes.
 * THE DEFINITION.  For one variant let m_r be stream r's metrics and t_r its status, r = 0..R-1, and s_r = eg_rank_score(m_r, mode).
 *   committed status    EG_EP_OK when every t_r is EG_EP_OK, otherwise t_r of the lowest r with t_r != EG_EP_OK: a variant is infeasible as
 *                       soon as one stream violates a constraint
 *   order of streams    worst first: a stream whose score is NaN ranks before every stream whose score is a number, then the smaller
 *                       score (-0.0 and +0.0 are equal), then the lower r.  The order covers all R streams, whatever their status
 *   committed metrics   for each i: of the `tail` worst streams, in ascending r, c = m_r[i] of the lowest selected r, then c = c + m_r[i]
 *                       for the others (plain double adds, one rounding each), then c / (double)tail.  tail == R is the mean outcome,
 *                       tail == 1 the worst stream's metrics bit for bit, anything between the mean of the worst tail (CVaR)
 *   eg_ensemble_row     nominal = m_0; committed as above; score_sum = s_0, then + s_r in ascending r; score_min / score_max the smallest /
 *                       largest s_r that is not NaN (the first of equal ones), both the quiet NaN 0x7FF8000000000000 when every s_r is
 *                       NaN; n_ok, n_infeasible the streams with t_r == EG_EP_OK, == EG_EP_INFEASIBLE, n_failed the others; worst_stream the
 *                       first stream of the order; status the committed status; pad zero
 * eg_plan_streams_validate: EG_ERR_BAD_ARG for n_streams outside 0..EG_STREAMS_MAX and, with n_streams >= 2, tail outside 1..n_streams or a
 * mode other than 1 | 2 (eg_rank_score's).  eg_plan_streams_set validates and stores the setting; n_streams 0 or 1 clears it (tail and mode
 * are then not read) and nothing runs differently from a context that never had one.  A rank of a group is refused.  Training batches
 * never see the setting.  eg_last_batch_streams returns the R the LAST batch ran under — 0 when it ran without streams, whatever is set
 * now; EG_ERR_BAD_ARG for a NULL context — with its tail and mode (either pointer may be NULL).  eg_fetch_plan_ensemble copies the n =
 * eg_last_batch_size() rows of it, eg_fetch_plan_streams every stream's metrics [R][n][4] and status [R][n] (either may be NULL);
 * both EG_ERR_BAD_ARG when the last batch ran without streams.
 * eg_repair_plans is refused while streams are set (EG_ERR_BAD_ARG): its pick reads the excess rows, which are stream 0's.  A chance level
 * for feasibility ("feasible in q of R") and streams on a group are not implemented.
 * Test hooks (they refuse a rank of a group): eg_debug_load_batch runs no passes; eg_debug_ensemble_keep copies the last batch's n records
 * into slab r (0..EG_STREAMS_MAX-1; the store is reserved for EG_STREAMS_MAX slabs of n), eg_debug_ensemble_commit runs k_ensemble_commit
 * over slabs 0..R-1 (R 1..EG_STREAMS_MAX) and the last batch's records, after which the two fetches serve it. */
#define EG_STREAMS_MAX 64
typedef struct { double nominal[4], committed[4]; double score_min, score_max, score_sum; int32_t n_ok, n_infeasible, n_failed, worst_stream;
                 int32_t status; int32_t pad[5]; } eg_ensemble_row;   /* 128 bytes */
int32_t eg_plan_streams_validate(int32_t n_streams, int32_t tail, int32_t mode);
int32_t eg_plan_streams_set(eg_ctx *, int32_t n_streams /* 0 or 1: clear */, int32_t tail /* 1..n_streams */, int32_t mode /* 1 | 2 */);
int32_t eg_last_batch_streams(const eg_ctx *, int32_t *tail, int32_t *mode);
int32_t eg_fetch_plan_ensemble(eg_ctx *, eg_ensemble_row *rows /* [n] */);
int32_t eg_fetch_plan_streams(eg_ctx *, double *metrics /* [R][n][4] or NULL */, int32_t *status /* [R][n] or NULL */);
int32_t eg_debug_ensemble_keep(eg_ctx *, int32_t r);
int32_t eg_debug_ensemble_commit(eg_ctx *, int32_t n_streams, int32_t tail, int32_t mode);

/* Breeding a front: generations of plan crosses with Pareto selection, the survivors' plan blocks becoming the next generation's parents
 * on the device.  eg_breed_plans(ctx, policy, opts, parents, breed_opts, seed, episode_index, ...) starts from the population P_0 = the
 * given 1..EG_CROSS_MAX_PARENTS plans, in order.  Generation g = 0, 1, ... :
 *   variants     with n = |P_g|: every parent first, as the cross {p, p, 0, 0} for p = 0..n-1; then {a, b, c, 26} for a, b != a and c of
 *                `cuts`, in lexicographic order (a, then b, then the position of c in `cuts`).  A cross whose child would hold more than
 *                4 096 entries in either list is removed and counted in n_skipped; the call is not refused.  A variant's NUMBER is its
 *                position in the list that remains;
 *   evaluation   chunk k holds the variants [k L, (k + 1) L), L = launch_variants (1..EG_CROSS_MAX_VARIANTS; 0 means
 *                EG_CROSS_MAX_VARIANTS).  Each chunk runs exactly as eg_evaluate_plan_crosses(..., first_episode_index = episode_index,
 *                same_index = 1) runs it over P_g, the per-variant short or long replay route included;
 *   selection    a private archive starts empty at every generation (it is NOT the context's eg_pareto_track archive, which stays
 *                untouched).  After every chunk it is folded with eg_pareto_track's definitions, word for word — valid, oriented
 *                dominance over `objectives`, the same point held once at the lowest index, the capacity rule with `mode` and the
 *                sticky n_dropped — the index of a variant being its number.  The archive after the last chunk, in ascending variant
 *                number, is P_{g+1}.  Parents have the lowest numbers, so a child that only equals a parent's point never displaces
 *                it; every parent is a variant, so the front never gets worse.  With n_dropped > 0 the result depends on the chunk
 *                boundaries, which L defines and which are therefore part of the contract; the call is deterministic either way;
 *   stop         EG_BREED_CONVERGED: P_{g+1} consists of exactly the n parents (n survivors, every number < n) — checked first;
 *                EG_BREED_MAX_GENERATIONS: max_generations generations have run;
 *                EG_BREED_EMPTY: no variant of the generation was valid; the population of that generation is returned.  (Only
 *                generation 0 can end so: a survivor was valid and is evaluated again as the same episode.)
 * Returned: *population = P_final (free with eg_plans_free; names ""), decoded from the population's blocks as they stand on the device
 * after the last generation — not rebuilt from the genealogy; generations[max_generations], a row per generation that ran;
 * members[max_generations][cap], the survivors of every generation in ascending variant number (`cross` is against P_g: the whole
 * genealogy); *n_generations; *stop_reason; out (cap episodes, may be NULL): the records of P_final's members, row r member r, taken
 * from the archive's record slots (not written after EG_BREED_EMPTY).
 * Per chunk the host uploads 8 bytes per variant and the routing; per generation it reads one buffer back (a row per survivor: number,
 * metrics, score and the block's two prefix-offset tables, from which the next generation is enumerated and routed).  No per-variant
 * data comes down and no plan block goes up after generation 0 (csrc/eg_breed.h k_breed_gather, k_breed_turnover).
 * Everything else is the contract of eg_evaluate_plan_crosses: no statistics, update or training folds, the resident policy untouched,
 * a rank of a group refused, the policy checked and staged once per call, the last launch's variants left behind as the last batch.
 * eg_breed_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the field for a parent set that is not a valid set of
 * 1..EG_CROSS_MAX_PARENTS plans, NULL options, a mode other than 1 or 2 (either with EG_PARETO_KEEP_SPREAD OR-ed in or not), objectives outside 1..15, cap outside 1..EG_PARETO_MAX,
 * max_generations < 1, launch_variants outside 0..EG_CROSS_MAX_VARIANTS, n_cuts outside 0..25, NULL cuts with n_cuts > 0, a cut outside
 * 1..25.  Nothing is launched after a refusal.
 * Under plan streams (eg_plan_streams_set, below) every chunk runs as R passes and the selection folds committed metrics and status: no other change. */
#define EG_BREED_CONVERGED 0
#define EG_BREED_MAX_GENERATIONS 1
#define EG_BREED_EMPTY 2
typedef struct { int32_t mode /* 1 | 2, | EG_PARETO_KEEP_SPREAD */, objectives /* 1..15 */, cap /* 1..EG_PARETO_MAX */, max_generations /* >= 1 */;
                 int32_t n_cuts; const uint8_t *cuts /* year indices 1..25; NULL with n_cuts 0: all 25 */;
                 int32_t launch_variants; } eg_breed_opts;
typedef struct { int32_t n_parents, n_skipped, n_kept, n_children_kept; int64_t n_variants, n_valid, n_dropped; } eg_breed_generation;   /* 40 bytes */
typedef struct { eg_plan_cross cross /* against P_g */; int32_t variant; double score, metrics[4]; } eg_breed_member;   /* 56 bytes */
int32_t eg_breed_validate(const eg_plan_set *parents, const eg_breed_opts *);
int32_t eg_breed_plans(eg_ctx *, const eg_policy_snapshot *policy, const eg_opts *, const eg_plan_set *parents, const eg_breed_opts *,
                       uint64_t seed, uint64_t episode_index, eg_plan_set **population, eg_breed_generation *generations /* [max_generations] */,
                       eg_breed_member *members /* [max_generations][cap] */, int32_t *n_generations, int32_t *stop_reason,
                       eg_episode_out *out /* cap rows, may be NULL */);

/* Exploring a front: a Pareto local search over one-entry edits and moves, the archive and its unexplored members kept on the device.
 * eg_refine_plans walks every plan of a front toward the same scalar optimum; eg_breed_plans recombines what a population holds.
 * eg_explore_plans(ctx, policy, opts, starts, explore_opts, seed, episode_index, ...) changes single entries and selects by dominance.
 *   neighbourhood  of a plan: the variants of one round of eg_refine_plans_moves for that plan (replace_with, append_with and max_shift
 *                of the options) WITHOUT its variant 0, in that order: the deletes of best_actions, the deletes of
 *                best_deficit_actions, the replaces, the appends (none while best_actions holds 4 096 entries), the moves;
 *   numbers      every variant of the call gets a NUMBER (int64); numbers count on from generation to generation;
 *   generation 0 the n start plans first, as "none" edits, numbers 0..n-1; then the neighbourhood of each start plan in order.  The
 *                frontier F_0 is the start plans;
 *   generation g > 0   the neighbourhoods of the members of F_g in ascending number, and nothing else.  M_g is the number of generation
 *                g's first neighbour (M_0 = n);
 *   evaluation   the generation's variants are cut into chunks of L = launch_variants (1..EG_CROSS_MAX_VARIANTS; 0 means
 *                EG_CROSS_MAX_VARIANTS); a cut falls anywhere, there are no segments: a variant carries the position of its base in the
 *                frontier array as its slot.  Each chunk runs as a launch of eg_refine_plans_moves runs — k_plan_edits_many writes the
 *                blocks, k_plan_moves behind it when the chunk holds a move, the plan batch with same_index = 1 at episode_index — the
 *                short or long replay route chosen per variant from the base's best_actions length plus the edit's delta;
 *   selection    ONE private archive per call (NOT the context's eg_pareto_track archive, which stays untouched): it starts empty at
 *                the call and is KEPT across generations.  After every chunk it is folded with eg_pareto_track's definitions, word for
 *                word — valid, oriented dominance over `objectives`, the same point held once at the lowest index, the capacity rule
 *                with `mode` and the sticky n_dropped — the index of a variant being its number.  Numbers only grow, so a neighbour that
 *                merely equals a held point never displaces it, and the front never gets worse.  With n_dropped > 0 the result depends
 *                on the chunk boundaries, which L defines and which are therefore part of the contract; the call is deterministic
 *                either way;
 *   frontier     F_{g+1} is the archive's entries with number >= M_g after the generation's last chunk: the members nobody has
 *                explored yet.  A member whose neighbourhood has been evaluated is never enumerated again.  A base that a neighbour
 *                dominates in the middle of a generation still has the rest of its neighbourhood evaluated: the frontier array is not
 *                touched during a generation;
 *   stop         checked in this order after a generation:
 *                EG_EXPLORE_EMPTY: no variant so far was valid (the archive is empty; generation 0 only).  The start plans are returned;
 *                EG_EXPLORE_EXPLORED: F_{g+1} is empty.  With n_dropped == 0 every member is then a Pareto local optimum of the
 *                neighbourhood;
 *                EG_EXPLORE_BUDGET: max_variants > 0, and the next generation's variant count plus those already run would exceed it;
 *                that generation is not started (generation 0 always runs);
 *                EG_EXPLORE_MAX_GENERATIONS: max_generations generations have run.
 * Returned: *population = the archive's plans in ascending number (free with eg_plans_free; names ""), decoded from the archive's block
 * slots as they stand on the device — not rebuilt from the genealogy; generations[max_generations], a row per generation that ran:
 * n_frontier = |F_g|, n_held and n_dropped = the archive's after the generation (n_dropped is the call's running total), n_new =
 * |F_{g+1}|, n_variants and n_valid = the generation's own; members[max_generations + 1][cap]: row 0 holds the start plans the archive
 * held after generation 0 (parent -1, a "none" edit, number = position in `starts`), row g + 1 holds F_{g+1} in ascending number —
 * `parent` is the number of the plan the edit or move is against, which stands in the row before (or is a start plan): the whole
 * genealogy; final_numbers[cap]: the numbers of *population's members, n_held of the last generation; *n_generations; *stop_reason;
 * out (cap episodes, may be NULL): the records of *population's members, row r member r, taken from the archive's record slots (not
 * written after EG_EXPLORE_EMPTY).
 * Per chunk the host uploads 8 bytes per variant, 4 for its slot, and the routing; per generation it reads one buffer back: a header
 * and a row for every NEW member only (number, metrics, score and the block's two prefix-offset tables, from which the next generation
 * is enumerated and routed — chunk by chunk: the host never holds a generation's variants, which can be tens of millions).  After
 * generation 0 the start plans the archive holds have rows too — they entered in it, and that is how row 0 of `members` is known.
 * After the last generation the archive's entries (56 bytes each) are read once.  No per-variant data comes down and no plan block goes up after
 * generation 0 (csrc/eg_breed.h k_breed_gather, csrc/eg_explore.h k_explore_turnover).
 * Everything else is the contract of eg_breed_plans: no statistics, update or training folds, the resident policy and the context's own
 * archives untouched, a rank of a group refused, the policy checked and staged once per call, the last launch's variants left behind
 * as the last batch.
 * eg_explore_validate runs the checks alone: EG_ERR_BAD_ARG with a message naming the field for a start set that is not a valid set of
 * 1..EG_CROSS_MAX_PARENTS plans, NULL options, a mode other than 1 or 2 (either with EG_PARETO_KEEP_SPREAD OR-ed in or not), objectives outside 1..15, cap outside 1..EG_PARETO_MAX,
 * max_generations < 1, n_replace or n_append < 0, a NULL list with a count, an action above 60, max_shift outside 0..25,
 * launch_variants outside 0..EG_CROSS_MAX_VARIANTS, max_variants < 0.  Nothing is launched after a refusal.
 * eg_explore_neighbourhood (host only, the same checks first): sizes[p] = the neighbourhood size of start plan p.
 * Under plan streams (eg_plan_streams_set, below) every chunk runs as R passes and the archive folds committed metrics and status: no other change. */
#define EG_EXPLORE_EXPLORED 0
#define EG_EXPLORE_MAX_GENERATIONS 1
#define EG_EXPLORE_EMPTY 2
#define EG_EXPLORE_BUDGET 3
typedef struct { int32_t mode /* 1 | 2, | EG_PARETO_KEEP_SPREAD */, objectives /* 1..15 */, cap /* 1..EG_PARETO_MAX */, max_generations /* >= 1 */;
                 int32_t n_replace; const uint8_t *replace_with; int32_t n_append; const uint8_t *append_with;
                 int32_t max_shift /* 0..25; 0: no moves */, launch_variants;
                 int64_t max_variants /* 0: no budget */; } eg_explore_opts;   /* 64 bytes */
typedef struct { int32_t n_frontier, n_held, n_new, pad; int64_t n_variants, n_valid, n_dropped; } eg_explore_generation;   /* 40 bytes */
typedef struct { int64_t parent /* a number; -1: a start plan */; int32_t is_move; eg_plan_edit edit; eg_plan_move move;
                 int64_t number; double score, metrics[4]; } eg_explore_member;   /* 88 bytes */
int32_t eg_explore_validate(const eg_plan_set *starts, const eg_explore_opts *);
int32_t eg_explore_neighbourhood(const eg_plan_set *starts, const eg_explore_opts *, int64_t *sizes /* [n_plans] */);
int32_t eg_explore_plans(eg_ctx *, const eg_policy_snapshot *policy, const eg_opts *, const eg_plan_set *starts, const eg_explore_opts *,
                         uint64_t seed, uint64_t episode_index, eg_plan_set **population,
                         eg_explore_generation *generations /* [max_generations] */,
                         eg_explore_member *members /* [max_generations + 1][cap] */, int64_t *final_numbers /* [cap] */,
                         int32_t *n_generations, int32_t *stop_reason, eg_episode_out *out /* cap rows, may be NULL */);

/* ---- eg_group: one process drives N ranks, one context per rank (no counterpart in the reference: the N-rank form of the
 * reduced-update loop above).  A group owns its contexts.  The exchange between ranks is inside the library — device-to-device
 * copies, no collective library — and every call enqueues the work of all ranks from the calling thread without synchronising
 * the host.
 *   eg_group_create    one context per entry of `devices` (repeats allowed: ranks that share a GPU); NULL + eg_last_error() when a
 *                      device does not exist
 *   eg_group_rank      a rank's context, for per-rank queries (eg_fetch, eg_timing_read, eg_memory_report, eg_fetch_best_run, ...);
 *                      it belongs to the group: never eg_destroy it, and its own best_result fold stays off (eg_best_result_track
 *                      refuses a rank)
 *   eg_group_push      eg_policy_push on every rank: every rank holds the same policy
 *   eg_group_step      one training step over the global batch of n_global episodes [first_episode_index, + n_global): rank r runs
 *                      the contiguous shard parallel.shard_range gives it (the first ranks take the remainder; shards may be empty),
 *                      every rank's update packet (and fold block) reaches every rank, and every rank applies the N packets —
 *                      replicas stay bit-identical, and equal to ONE context's eg_device_step over the same batches.  replay_period
 *                      and noise_seed as for eg_device_step
 *   eg_group_pull      eg_policy_pull from one rank (they all hold the same policy)
 *   eg_group_replay_hoist  eg_replay_hoist on every rank
 *   eg_group_best_result_track / eg_group_fetch_best_result   the reference's best_result fold (see eg_best_result_track) over the
 *                      results of ALL ranks in global index order: exactly one context's fold over the same episodes.  The fold's
 *                      state is kept on every rank; the held run's record only by the rank that ran it, and fetched from there.
 *   eg_group_top_k_track / eg_group_fetch_top_k   the top-K archive (see eg_top_k_track) over the results of ALL ranks: exactly one
 *                      context's archive over the same episodes.  Each rank sends its shard's own top-k distinct entries behind its
 *                      message; every rank merges the N blocks into its replica of the archive; an entry's record is kept by the rank
 *                      that ran it, and fetched from there. */
typedef struct eg_group eg_group;
eg_group *eg_group_create(const int32_t *devices, int32_t n_ranks, const eg_world *world);
void eg_group_destroy(eg_group *);
eg_ctx *eg_group_rank(eg_group *, int32_t rank);
int32_t eg_group_push(eg_group *, const eg_policy *, const eg_opts *opts);
int32_t eg_group_step(eg_group *, uint64_t seed, uint64_t first_episode_index, uint32_t n_global, uint32_t replay_period,
                      uint64_t noise_seed);
int32_t eg_group_pull(eg_group *, int32_t rank, eg_policy *);
int32_t eg_group_replay_hoist(eg_group *, int32_t on);
int32_t eg_group_best_result_track(eg_group *, int32_t mode);
int32_t eg_group_fetch_best_result(eg_group *, eg_episode_out *out, int32_t *state, int64_t *global_index);
int32_t eg_group_top_k_track(eg_group *, int32_t k, int32_t mode);
int32_t eg_group_fetch_top_k(eg_group *, eg_episode_out *out, int32_t *n_held, double *scores, int64_t *global_index);

/* Test hook: fills the LDS of every compute unit with `value` and waits.  LDS is not cleared between workgroups, so a
 * kernel that reads a word before writing it sees what the previous tenant left; the parity tests call this with small
 * integers (the values the helper protocol's sequence flags take) before a rollout. */
int32_t eg_debug_fill_lds(eg_ctx *, uint32_t value);
/* Test hooks: a crafted batch, and the reductions that decide what a run keeps over it — ties, staircases, NaN and infinities, key
 * edges, maxima on wave and stride boundaries: what real episodes never produce.  Host code only; every kernel is the one a run launches.
 * All of them refuse a rank of a group.
 *   eg_debug_load_batch   makes the context's record buffer a batch of n synthetic records — sized as a launch of n would size it;
 *                         eg_last_batch_size() = n, global indices first_index + e.  Record e is zero except: metrics[e], status[e];
 *                         n_draws = g = first_index + e as a tag; n_run[0] = n_def[0] = EG_DEBUG_LIST_LEN with run_log[0..8) the bytes of g
 *                         and def_log[0..8) the bytes of ~g (little-endian), so that a copied list shows its source; n_act[e] and the
 *                         WHOLE act_log row as given, the bytes behind the log's length included (NULL: zeros); and score_list[e], the
 *                         back-to-back scores of the statistics epilogue (NULL: zeros).
 *   eg_debug_fold_last_batch   runs, on the last batch, exactly what a training batch runs behind its rollout for the folds `what`
 *                         selects (EG_DEBUG_FOLD_BEST_RESULT | EG_DEBUG_FOLD_TOP_K; the fold's tracking must be on).  use_score_list:
 *                         the top-K fold takes its rank scores from score_list, as behind a batch whose statistics epilogue ran (mode 1).
 *   eg_debug_pick_best    k_pick_best over the last batch into the context's update packet; `candidate` receives the candidate record
 *                         (EG_CANDIDATE_BYTES, layout above).  The contract of score_list: the epilogue writes score_metrics (>= 0) for an
 *                         episode that ended EG_EP_OK and -1.0 for a failed one; the pick is the FIRST maximum among the scores above
 *                         -1.0 (a NaN never compares above anything), and score -1.0 / index -1 when there is none.
 *   eg_debug_refine_pick  k_refine_pick_many over the last batch as ONE segment (n <= EG_REFINE_MAX_VARIANTS records = variants:
 *                         eg_debug_refine_pick_many with the segment [0, n), as eg_refine_plan launches the kernel) with n plan blocks,
 *                         a base block and n packed edits of the hook's own: block j is the 32-bit words j * 0x9E3779B1 + w (w = 0 ..
 *                         EG_PLAN_BLOCK_BYTES / 4) with the two list totals (words 130 and 158: entry [26] of the prefix offsets)
 *                         j mod 4097 and (j / 3) mod 4097; the base block is the words 0xBA5E0000 + w with totals 7 and 5; edit j is
 *                         (j, ~j).  `entry` receives the step entry (EG_DEBUG_REFINE_ENTRY_BYTES: i32 winner, n_failed | u32 edit[2] |
 *                         f64 score, metrics[4] | i32 off26, offd26, base_ok, n | f64 base_score, base_metrics[4]), `base_block` the base
 *                         block as the kernel left it.
 *   eg_debug_refine_pick_many  k_refine_pick_many over the last batch cut into n_segs segments (1..EG_REFINE_MAX_PLANS; segment s is the
 *                         records [seg_first[s], + seg_count[s]); the segments must tile [0, n) in order): plan block j, the packed
 *                         edits (j, ~j) and the list totals as for eg_debug_refine_pick; base block s is the words 0xBA5E0000 + (s << 8)
 *                         + w with totals 7 and 5.  `entries` receives n_segs step entries of EG_DEBUG_REFINE_ENTRY_BYTES (`winner`
 *                         relative to the segment), `base_blocks` the n_segs base blocks as the kernel left them.
 *   eg_debug_repair_pick_many  k_repair_pick_many the same way — the segments, the tagged plan blocks, packed edits, list totals and base
 *                         blocks of eg_debug_refine_pick_many — over the last batch as eg_debug_constrain_last_batch judged it (behind
 *                         eg_debug_load_batch and eg_debug_load_yearly), under the k constraints it was judged under and `weights`
 *                         ([k], each finite and > 0; NULL: 1.0 each).  EG_ERR_BAD_ARG when the last batch was not judged.  `entries`
 *                         receives n_segs entries of EG_DEBUG_REPAIR_ENTRY_BYTES: i32 winner (-1: the base is no candidate; 0: V_0 == 0,
 *                         or no candidate lies below V_0), n_failed | u32 edit[2] | f64 violation, score, metrics[4] — the winner's;
 *                         for winner 0 the base's; for winner -1 zeros and variant 0's metrics — | u32 violated | i32 n_feasible, off26,
 *                         offd26, base_ok, n | f64 base_violation, base_score | u32 base_violated, 0 — the base's three are zeros when
 *                         it is no candidate. */
#define EG_DEBUG_LIST_LEN 8
#define EG_DEBUG_FOLD_BEST_RESULT 1
#define EG_DEBUG_FOLD_TOP_K 2
#define EG_DEBUG_REFINE_ENTRY_BYTES 112
int32_t eg_debug_load_batch(eg_ctx *, const double *metrics /* [n][4] */, const int32_t *status /* [n] */, const int32_t *n_act /* [n][26] or NULL */,
                            const uint8_t *act_log /* [n][EG_ACT_CAP] or NULL */, const double *score_list /* [n] or NULL */, uint32_t n,
                            uint64_t first_index);
int32_t eg_debug_fold_last_batch(eg_ctx *, int32_t what, int32_t use_score_list);
int32_t eg_debug_pick_best(eg_ctx *, void *candidate /* EG_CANDIDATE_BYTES */);
int32_t eg_debug_refine_pick(eg_ctx *, int32_t mode /* 1 | 2 */, void *entry /* EG_DEBUG_REFINE_ENTRY_BYTES */, uint8_t *base_block /* EG_PLAN_BLOCK_BYTES */);
int32_t eg_debug_refine_pick_many(eg_ctx *, int32_t mode, const uint32_t *seg_first, const uint32_t *seg_count, int32_t n_segs,
                                  void *entries /* n_segs * EG_DEBUG_REFINE_ENTRY_BYTES */, uint8_t *base_blocks /* n_segs * EG_PLAN_BLOCK_BYTES */);
#define EG_DEBUG_REPAIR_ENTRY_BYTES 112
int32_t eg_debug_repair_pick_many(eg_ctx *, int32_t mode, const double *weights /* [k] or NULL */, const uint32_t *seg_first, const uint32_t *seg_count,
                                  int32_t n_segs, void *entries /* n_segs * EG_DEBUG_REPAIR_ENTRY_BYTES */,
                                  uint8_t *base_blocks /* n_segs * EG_PLAN_BLOCK_BYTES */);
/* Test hooks: a crafted generation of eg_breed_plans / eg_explore_plans without a rollout — synthetic records and tagged plan blocks
 * folded into the calls' private archive and turned over by the kernels the two calls launch (k_pareto_filter .. k_pareto_finalize,
 * k_breed_gather, k_breed_turnover, k_explore_turnover), through the launch helpers they use, in their order, on the null stream.  The
 * context's own archive (eg_pareto_track, eg_fetch_pareto) is not touched.  All of them refuse a rank of a group; chunk, turnover and
 * fetch refuse a context on which eg_debug_breed_begin has not succeeded; a refusal launches nothing.
 *   eg_debug_breed_begin     reserves the private archive as eg_breed_plans does and starts it: an empty state with cap (1..EG_PARETO_MAX),
 *                            objectives (1..15) and mode (1 | 2, EG_PARETO_KEEP_SPREAD OR-ed in or not), zero counters, and every byte of the record slots, the block slots, the
 *                            two parent / frontier arrays and the readback buffer EG_DEBUG_BREED_CANARY.
 *   eg_debug_breed_chunk     one chunk of a generation, n variants (1..EG_CROSS_MAX_VARIANTS) numbered first_index ..: eg_debug_load_batch(ctx,
 *                            metrics, status, NULL, NULL, NULL, n, first_index) — the tag n_draws of record j is its number g = first_index
 *                            + j —, n plan blocks into the plan pool, the fold, k_breed_gather.  32-bit word w of block j (w = 0 ..
 *                            EG_PLAN_BLOCK_BYTES / 4) is ((g * EG_DEBUG_BREED_TAG_MUL mod 2^64) >> 32) + w mod 2^32: consecutive inside a
 *                            block, and the block's first word a Fibonacci hash of the whole 64-bit number.
 *   eg_debug_breed_turnover  kind EG_DEBUG_TURNOVER_BREED: k_breed_turnover into parent array `next` (0 | 1; m_first is not read);
 *                            kind EG_DEBUG_TURNOVER_EXPLORE: k_explore_turnover into frontier array `next` with m_first (>= 0).
 *   eg_debug_breed_fetch     copies down whatever is not NULL: `state` (EG_DEBUG_PARETO_STATE_BYTES: i32 cap, n_held, objectives, mode | i64
 *                            n_dropped, pad | EG_PARETO_MAX entries of EG_DEBUG_PARETO_ENTRY_BYTES: f64 metrics[4], score | i64 index | i32
 *                            slot, pad), the EG_PARETO_MAX block slots, the two parent / frontier arrays (EG_PARETO_MAX blocks each), the
 *                            readback buffer (EG_DEBUG_BREED_READBACK_BYTES: a header of EG_DEBUG_BREED_HEADER_BYTES — i32 n_held, i32 0
 *                            (explore: n_new) | i64 n_dropped, n_valid, 0 — then EG_PARETO_MAX rows of EG_DEBUG_BREED_ROW_BYTES: the entry,
 *                            zeros up to byte 64, then the EG_DEBUG_BREED_ROW_BYTES - 64 bytes of the block from byte
 *                            EG_DEBUG_BREED_BLOCK_OFFSETS on, its two prefix-offset tables), the counters (u64 n_valid | u32 done, pad) and
 *                            the tag n_draws of each of the EG_PARETO_MAX record slots. */
#define EG_DEBUG_BREED_CANARY 0xC5
#define EG_DEBUG_BREED_TAG_MUL 0x9E3779B97F4A7C15ull
#define EG_DEBUG_TURNOVER_BREED 1
#define EG_DEBUG_TURNOVER_EXPLORE 2
#define EG_DEBUG_PARETO_ENTRY_BYTES 56
#define EG_DEBUG_PARETO_STATE_BYTES (32 + EG_PARETO_MAX * EG_DEBUG_PARETO_ENTRY_BYTES)
#define EG_DEBUG_BREED_HEADER_BYTES 32
#define EG_DEBUG_BREED_ROW_BYTES 288
#define EG_DEBUG_BREED_READBACK_BYTES (EG_DEBUG_BREED_HEADER_BYTES + EG_PARETO_MAX * EG_DEBUG_BREED_ROW_BYTES)
#define EG_DEBUG_BREED_BLOCK_OFFSETS 416
int32_t eg_debug_breed_begin(eg_ctx *, int32_t cap, int32_t objectives, int32_t mode);
int32_t eg_debug_breed_chunk(eg_ctx *, const double *metrics /* [n][4] */, const int32_t *status /* [n] */, uint32_t n, uint64_t first_index);
int32_t eg_debug_breed_turnover(eg_ctx *, int32_t kind, int32_t next, int64_t m_first);
int32_t eg_debug_breed_fetch(eg_ctx *, void *state /* EG_DEBUG_PARETO_STATE_BYTES */, uint8_t *blocks /* EG_PARETO_MAX * EG_PLAN_BLOCK_BYTES */,
                             uint8_t *array0 /* EG_PARETO_MAX * EG_PLAN_BLOCK_BYTES */, uint8_t *array1 /* likewise */,
                             uint8_t *readback /* EG_DEBUG_BREED_READBACK_BYTES */, void *counters /* 16 bytes */, uint64_t *tags /* [EG_PARETO_MAX] */);
/* Test hook: the lazy penalty field's catch-up (csrc/eg_field.h tiles_refresh) for ONE pair of tiles on one wave, as a search of
 * k_replay_lazy calls it, against a crafted generator list.  `cells`: the list, n_cells (0..EG_MAX_GENS) grid cells i * EG_GRID + j in
 * list order (the first EG_ONCHIP_GENS go to LDS, the rest are read where a record keeps them); radius_class 0..5 (one a generator
 * type has); tile_a 0..EG_DEBUG_TILES - 1, tile_b likewise and not tile_a, or -1: none (tile t covers the rows (t / 7) * 8 .. + 7 and
 * the columns (t % 7) * 8 .. + 7 of the grid, edge tiles 3 wide).  `field`, in and out, is the class's field as a slot of the pool holds
 * it: EG_DEBUG_FIELD_DOUBLES doubles — the value of cell c at [c], and from double EG_DEBUG_TILE_COUNTERS on, as 16-bit words, how many
 * generators of the list each tile's stored values hold (0: none, the values count as 1.0 whatever is stored).  On return the two
 * tiles' values are current, their counters n_cells, and nothing else has changed.  `folded`: the generators the call folded (one
 * that both tiles need counts once).  Refuses a rank of a group. */
#define EG_DEBUG_FIELD_DOUBLES 2624
#define EG_DEBUG_TILE_COUNTERS 2602
#define EG_DEBUG_TILES 49
#define EG_DEBUG_TILE_WIDTH 8
int32_t eg_debug_tiles_refresh(eg_ctx *, const uint16_t *cells /* [n_cells] */, int32_t n_cells, int32_t radius_class, int32_t tile_a, int32_t tile_b,
                               double *field /* EG_DEBUG_FIELD_DOUBLES */, int32_t *folded);
/* Diagnostic hook: ONE idle workgroup of 256 threads on the library's side stream that stays resident for `cycles` shader cycles;
 * variant 0: 1 KB of LDS, few registers; 1: 150 KB of LDS; 2: 200+ registers a lane; 3: both (the hoisted replay's footprint).  What a
 * resident workgroup costs the grid beside it: scripts/side_kernel_probe.py, profiles/r04_ab_notes.log. */
int32_t eg_debug_occupy(eg_ctx *, int32_t variant, uint64_t cycles);

/* B2: one placement search on the device (settlements of year index `year_index`, the ctx's existing plant plus
 * `n_extra` generators given by grid cell), for parity tests of the arg-max kernel. */
int32_t eg_place(eg_ctx *, int32_t gen_type, int32_t year_index, const uint16_t *extra_cells, int32_t n_extra /* <= EG_ONCHIP_GENS */,
                 int32_t *out_cell, double *out_score);

/* B2 with the reference's own signature — MetalLocationSearch::find_suitable_location(&self, settlements, generators,
 * coastline_points, gen_type, size_penalty: f32) -> Option<Coordinate> (gpu/metal_location_search.rs:96-103): the settlements
 * (with the populations of year `year_index`), the existing plant and the coastline are the ctx's world; `gen_x / gen_y` are
 * the further generators of the caller's map at ARBITRARY coordinates (metres), in list order.  *found = 0 is the
 * reference's None; otherwise (*out_x, *out_y) is the winning candidate's coordinate as Coordinate::new clamps it. */
int32_t eg_find_suitable_location(eg_ctx *, int32_t year_index, int32_t gen_type, const double *gen_x, const double *gen_y,
                                  int32_t n_generators, float size_penalty, double *out_x, double *out_y, int32_t *found,
                                  double *out_score /* may be NULL */);

/* ---- policy-independent host tables (built once per world; no device needed), read-only views for validation.
 * Names: usage population pre_co2 pre_tg pre_ig pre_sg pre_optot te coastf dr m03 t12 cc out_mw co2_t offv offc
 * inflation carbon_price size_factor (f64); pre_opcnt cls rclass marine reach existing_online (i32). ---- */
typedef struct eg_host_tables eg_host_tables;
eg_host_tables *eg_host_tables_create(const eg_world *world);
void eg_host_tables_free(eg_host_tables *);
int32_t eg_host_tables_f64(const eg_host_tables *, const char *name, const double **ptr, int64_t *len);
int32_t eg_host_tables_i32(const eg_host_tables *, const char *name, const int32_t **ptr, int64_t *len);

/* ---- ActionWeights on the host (C++ mirror of ai/learning/weights/) ---- */
eg_policy *eg_policy_new(void);                                     /* core.rs:25-250 */
void eg_policy_free(eg_policy *);
int32_t eg_policy_snapshot_view(const eg_policy *, eg_policy_snapshot *out);  /* pointers live as long as the policy */
int32_t eg_policy_get_tables(const eg_policy *, double *w, double *dw, double *cw);
int32_t eg_policy_set_tables(eg_policy *, const double *w, const double *dw, const double *cw);
double eg_policy_get_scalar(const eg_policy *, int32_t which);     /* same codes as the oracle: see eg_policy.cpp */
int32_t eg_policy_set_scalar(eg_policy *, int32_t which, double v);
int32_t eg_policy_get_list(const eg_policy *, int32_t which, int32_t year_index, uint8_t *out, int32_t cap);
/* multi_simulation.rs:494-508 for one episode: transfer_recorded_actions_from → apply_contrast_learning →
 * update_best_strategy → apply_deficit_contrast_learning.  run/def lists are flat year-major with counts. */
int32_t eg_policy_apply_episode(eg_policy *, const double metrics[4], const int32_t *n_run, const uint8_t *run_log,
                                const int32_t *n_def, const uint8_t *def_log, uint64_t noise_seed);
/* The same three steps for a whole batch that shared one snapshot: `stats` is the (all-reduced) host copy of the
 * eg_update_stats buffer, the candidate is the batch's best episode (highest score, ties to the lowest global index). */
int32_t eg_policy_apply_reduced(eg_policy *, const int64_t *stats, const double cand_metrics[4], const int32_t *cand_n_run,
                                const uint8_t *cand_run_log, const int32_t *cand_n_def, const uint8_t *cand_def_log,
                                uint64_t noise_seed);
/* The same update from update packets: `stats` = the (all-reduced) int64[EG_STATS_LEN] statistics, `candidates` =
 * n_candidates candidate records of EG_CANDIDATE_BYTES each (one per rank, in rank order; layout above).  The winner is
 * the record with the highest score, ties to the lowest global index (index < 0: no candidate).  Returns 1 when the
 * winner became the best strategy, 0 when not, < 0 on error. */
int32_t eg_policy_apply_packet(eg_policy *, const int64_t *stats, const void *candidates, int32_t n_candidates,
                               uint64_t noise_seed);
/* One whole pass of the batch training step on one GPU, one call: snapshot upload, rollout with the statistics
 * epilogue, best pick, ONE packet copy to pinned host memory, eg_policy_apply_packet.  Same return convention. */
int32_t eg_train_step(eg_ctx *, eg_policy *, const eg_opts *opts, uint64_t seed, uint64_t first_episode_index,
                      uint32_t n_episodes, const uint8_t *replay_mask /* host, may be NULL */, uint64_t noise_seed);
/* Device-resident policy.  eg_policy_push uploads the policy once; after that every training step runs on the device with
 * no host synchronisation: eg_device_rollout enqueues the rollout (statistics epilogue, best pick) into `d_packet`
 * (DEVICE, EG_PACKET_BYTES, zeroed once by the caller); eg_device_apply enqueues the batch update from n_packets update
 * packets laid out back to back (DEVICE; with one GPU that is d_packet itself, with N GPUs the result of ONE all-gather of
 * every rank's packet on the same stream — the statistics are integer sums, so adding them up in the kernel is the
 * all-reduce) and zeroes the statistics of `d_own_packet` for the next step.  eg_device_step does both on a
 * library-owned packet (one GPU).  The update is the one of eg_policy_apply_packet, bit for bit (both evaluate
 * csrc/eg_reduced_math.h).  replay_period > 0: the episode with global index i replays the best strategy when
 * i % replay_period == 0 and a best strategy exists (decided on the device).  eg_policy_pull waits for the stream and
 * copies the policy back into `policy` (tables, counters, the best strategy if an on-device update installed one since
 * the push; improvement-history records are appended once per context, to whichever policy pulls first). */
int32_t eg_policy_push(eg_ctx *, const eg_policy *, const eg_opts *opts);
int32_t eg_device_rollout(eg_ctx *, uint64_t seed, uint64_t first_episode_index, uint32_t n_episodes, uint32_t replay_period,
                          void *d_packet);
int32_t eg_device_apply(eg_ctx *, const void *d_packets, int32_t n_packets, void *d_own_packet, uint64_t noise_seed);
int32_t eg_device_step(eg_ctx *, uint64_t seed, uint64_t first_episode_index, uint32_t n_episodes, uint32_t replay_period,
                       uint64_t noise_seed);
int32_t eg_policy_pull(eg_ctx *, eg_policy *);
/* Measurement support (no counterpart in the reference): eg_policy_hold keeps a copy of the device-resident policy as it is
 * now — tables, best strategy, counters — on the device, stream-ordered; eg_policy_rewind puts that copy back.  bench.py
 * rewinds before every batch, so that every batch is the same work on any number of GPUs: left to itself the training loop
 * changes what a replay episode costs, differently for every global batch size. */
int32_t eg_policy_hold(eg_ctx *);
int32_t eg_policy_rewind(eg_ctx *);
/* Replay hoist (no counterpart in the reference — it runs every iteration on its own, core/multi_simulation.rs:425-472).  An episode
 * with replay_best_strategy = true takes every action from the stored lists and reads no seeded draw until a list runs out
 * (ai/learning/weights/sampling.rs:78-101, :242-266; core/simulation.rs:146-162), so all replay episodes of a batch are one and the
 * same computation.  With the hoist on (eg_replay_hoist(ctx, 1), or EIRGRID_REPLAY_HOIST=1 in the environment at eg_create; off by
 * default) a batch computes that script ONCE — one cooperative workgroup of EG_COOP_WAVES waves, csrc/eg_replay_coop.h — and hands every replay
 * episode of the batch a copy of the record; records, statistics and update packets are those of the per-episode path, byte for byte
 * (n_chunks excepted: it counts what the search that really ran requested).  A script that needs a fallback draw
 * (sampling.rs:445-528) or would end with a status other than EG_EP_OK is not hoisted: the per-episode kernels run those episodes as
 * before.  eg_replay_hoist_stats waits for the device: *batches_armed = batches launched with the hoist on and replay episodes in
 * them, *last_batch_hoisted = 1 when the last such batch was served by the hoist. */
int32_t eg_replay_hoist(eg_ctx *, int32_t on);
int32_t eg_replay_hoist_stats(eg_ctx *, uint64_t *batches_armed, int32_t *last_batch_hoisted);
/* Diagnostic hook: cycle counts of the hoisted script's phases as a -DEG_COOP_STAMPS build of the library leaves them (zeros in the
 * shipped build): between commands, year start (own chains), waiting for the other waves' chains, command barrier, search, field update. */
int32_t eg_debug_hoist_stamps(eg_ctx *, uint64_t stamps[8]);
/* Checkpoints in the reference's JSON schema (SerializableWeights, ai/learning/serialization.rs:38-51):
 * save_to_file / load_from_file of ai/learning/weights/serialization.rs:29-493.  As in the reference the count table
 * is not part of the file; a loaded policy samples the action count with the heuristic branch (sampling.rs:423-442). */
int32_t eg_policy_save_json(const eg_policy *, const char *path);
eg_policy *eg_policy_load_json(const char *path);
/* --track-weight-history (core/multi_simulation.rs:166-207): append one snapshot {best_score, iteration, timestamp,
 * weights: ActionWeights::to_json()} to the pretty-printed JSON array in `path` (created as needed). */
int32_t eg_policy_append_weight_history(const eg_policy *, const char *path, uint64_t iteration);
/* improvement_history.csv of the reference's best-run export (utils/csv_export.rs:155-207); no file if there is no history */
int32_t eg_policy_export_improvement_csv(const eg_policy *, const char *path);   /* NULL + eg_last_error() on failure */
/* simulation_summary.csv of the best-run export (utils/csv_export.rs:215-432): final metrics, the action list with the
 * exporter's cost estimates, the yearly summary rows.  `run` holds one episode (metrics, yearly, n_act, act_log). */
int32_t eg_export_summary_csv(const eg_episode_out *run, const char *path, const char *timestamp);
/* The detail files of the same export (utils/csv_export.rs:434-1230, called from core/multi_simulation.rs:852-905):
 * <out_dir>/yearly_details/{settlements,generators,carbon_offsets}.csv and <out_dir>/operation_logs/generator_operation_logs.csv,
 * from the best episode's record (`run`: n_gens, gen_pack, n_act, act_log are read) and the world.  Host code, no device.
 * settlement_names: [n_settlements] or NULL ("Settlement_<i>").  offset_seed: carbon-offset coordinates come from thread_rng in
 * the reference (core/actions.rs:142-145); here from StdRng::seed_from_u64(offset_seed).  What the reference really writes —
 * and therefore this function — is described at the top of csrc/eg_export.cpp. */
int32_t eg_export_run_details(const eg_world *world, const char *const *settlement_names, const eg_episode_out *run,
                              const char *out_dir, uint64_t offset_seed);
double eg_score_metrics(const double metrics[4], int32_t cost_only);   /* ai/metrics/scoring.rs:5-45 */

#ifdef __cplusplus
}
#endif
#endif
