// eg_cli.h — what the units of the eirgrid-hip driver share: the arguments and the loaded world (eg_cli.cpp fills them), the handles a run
// holds of the library, an owned episode record with its export, and the small file, time and CSV helpers.  eg_cli.cpp: arguments, world,
// the training run; eg_cli_plans.cpp: the runs over given plans (--evaluate, --sensitivity, --refine).
#pragma once
#include <chrono>
#include <cstdio>
#include <ctime>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "eirgrid_hip.h"

struct Args {   // cli/cli.rs:5-59
  uint64_t iterations = 1000; bool parallel = true; bool no_continue = false; std::string checkpoint_dir = "checkpoints";
  uint64_t checkpoint_interval = 5; uint64_t progress_interval = 10; std::string cache_dir = "cache";
  bool force_full_simulation = false, enable_timing = false; bool has_seed = false; uint64_t seed = 0;
  bool verbose_state_logging = false, cost_only = false, enable_energy_sales = true, enable_csv_export = true;
  bool debug_logging = false, debug_weights = false, enable_construction_delays = false, track_weight_history = false;
  // engine-specific
  std::string world_json, assets_dir = "aiSimulator/assets"; uint32_t batch = 1024; std::string update = "reduced"; int device = 0;
  bool existing_operational_at_start = false;
  uint64_t stop_after = 0;      // leave the loop (as an interrupt would) once this many iterations are done and checkpointed
  std::string dump_world;       // write the loaded world (eirgrid_amd JSON form) there and exit: no device needed
  bool replay_hoist = true;     // the replay iterations of a batch computed once (eg_replay_hoist): the same results, the replay phases 5x faster
  // --gpus N / --devices LIST: the ranks of a multi-GPU run (eg_group), one device each; empty: the single-device run on --device
  std::vector<int32_t> ranks; bool device_given = false, gpus_given = false;
  int32_t top_k = 0;            // --top-k K: keep the K best distinct scenarios of the run (eg_top_k_track) and export them; 0: off
  std::string evaluate;         // --evaluate FILE: score the plans of FILE (eg_evaluate_plans) and exit; no training
  std::string evaluate_policy;  // --evaluate-policy CKPT: the policy the plans are evaluated under (default: ActionWeights::new)
  std::string sensitivity;      // --sensitivity FILE: score every one-entry edit of FILE's first plan (eg_evaluate_plan_edits) and exit
  std::vector<uint8_t> sensitivity_replace;      // --sensitivity-replace a,b,...: also every best_actions entry replaced by each of these
  std::string refine;           // --refine FILE: apply the best one-entry edit of FILE's plan round after round (eg_refine_plan) and exit
  int32_t refine_rounds = 64; bool refine_rounds_given = false;      // --refine-rounds N: at most N applied edits
  std::vector<uint8_t> refine_replace, refine_append;      // --refine-replace / --refine-append a,b,...: the moves beside the deletes
};

struct WorldData {
  std::vector<double> sx, sy; std::vector<uint32_t> spop; std::vector<double> gx, gy, gcap; std::vector<int32_t> gtype; std::vector<double> cx, cy;
  std::vector<std::string> names;      // settlement names (settlements.csv of the export); empty: "Settlement_<i>"
  eg_world view(bool at_start) const {
    eg_world w{}; w.n_settlements = int32_t(sx.size()); w.settlement_x = sx.data(); w.settlement_y = sy.data(); w.settlement_pop = spop.data();
    w.n_existing = int32_t(gx.size()); w.existing_x = gx.data(); w.existing_y = gy.data(); w.existing_type = gtype.data(); w.existing_capacity_mw = gcap.data();
    w.n_coast = int32_t(cx.size()); w.coast_x = cx.data(); w.coast_y = cy.data(); w.existing_operational_at_start = at_start ? 1 : 0; return w;
  }
};

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, eg_last_error()); return 1; } } while (0)

inline bool read_file(const std::string& path, std::string& out) {
  std::ifstream f(path, std::ios::binary); if (!f) return false;
  std::stringstream ss; ss << f.rdbuf(); out = ss.str(); return true;
}
inline bool exists(const std::string& p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }
inline std::string mkdirs(const std::string& p) {      // every directory of the path; gives the path back
  std::string cur;
  for (size_t i = 0; i <= p.size(); ++i) { if (i == p.size() || p[i] == '/') { if (!cur.empty()) ::mkdir(cur.c_str(), 0755); } if (i < p.size()) cur += p[i]; }
  return p;
}
constexpr const char* kStamp = "%Y%m%d_%H%M%S";      // the name of a directory made at the time of export (csv_export.rs:114-127)
inline std::string time_stamp(const char* fmt) { char buf[32]; std::time_t t = std::time(nullptr); std::tm tmv; localtime_r(&t, &tmv); std::strftime(buf, sizeof(buf), fmt, &tmv); return buf; }
using Clock = std::chrono::steady_clock;
inline double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }
// n numbers, round-trip exact, as a CSV row has them
inline std::string csv17(const double* v, int n, const char* sep = ",") {
  std::string s; char buf[40];
  for (int i = 0; i < n; ++i) { std::snprintf(buf, sizeof(buf), "%.17g", v[i]); s += i ? sep : ""; s += buf; }
  return s;
}

// What a run holds of the library, released on every way out (it is neither copied nor moved).  open() is the start of a run over given
// plans, after the run has validated its input: the policy (--evaluate-policy's checkpoint, or a fresh one), then the context on --device,
// and what every evaluation of the run is called with.
struct Session {
  eg_policy* policy = nullptr; eg_ctx* ctx = nullptr; eg_group* group = nullptr; eg_plan_set* plans = nullptr;
  eg_opts opts{}; eg_policy_snapshot snap{}; int mode = 1;      // (mode: eg_rank_score's, 2 with --cost-only)
  Session() = default; Session(const Session&) = delete; Session& operator=(const Session&) = delete;
  ~Session() { eg_policy_free(policy); eg_destroy(ctx); eg_group_destroy(group); eg_plans_free(plans); }
  int create(const Args& a, const eg_world& world) {      // the context alone; like open(), 0 or the exit code
    if (!(ctx = eg_create(a.device, &world))) std::fprintf(stderr, "eg_create: %s\n", eg_last_error());
    return ctx ? 0 : 1;
  }
  int open(const Args& a, const eg_world& world) {
    policy = a.evaluate_policy.empty() ? eg_policy_new() : eg_policy_load_json(a.evaluate_policy.c_str());
    if (!policy) { std::fprintf(stderr, "error: %s\n", eg_last_error()); return 1; }
    if (int rc = create(a, world)) return rc;
    mode = a.cost_only ? 2 : 1;
    opts = eg_opts{a.enable_energy_sales ? 1 : 0, 0, 1};
    CHECK(eg_policy_snapshot_view(policy, &snap));
    return 0;
  }
};

// K episode records with what the exports read (metrics, yearly rows, action log, generators), and record r as the library fills and reads it
struct Records {
  std::vector<double> metrics, yearly; std::vector<int32_t> n_act, n_gens; std::vector<uint8_t> act_log; std::vector<uint16_t> gen_pack;
  explicit Records(size_t K) : metrics(K * 4), yearly(K * EG_YEARS * EG_YEARLY_FIELDS), n_act(K * EG_YEARS), n_gens(K), act_log(K * EG_ACT_CAP), gen_pack(K * EG_MAX_GENS) {}
  eg_episode_out view(size_t r = 0) {
    eg_episode_out v{}; v.metrics = &metrics[r * 4]; v.yearly = &yearly[r * EG_YEARS * EG_YEARLY_FIELDS]; v.n_act = &n_act[r * EG_YEARS];
    v.act_log = &act_log[r * EG_ACT_CAP]; v.n_gens = &n_gens[r]; v.gen_pack = &gen_pack[r * EG_MAX_GENS]; return v;
  }
};
// one exported run in `dir`: simulation_summary.csv, yearly_details/ and operation_logs/ (csrc/eg_export.cpp), as the best run's export writes them
inline int export_entry(const eg_world& world, const WorldData& wd, const eg_episode_out& view, const std::string& dir, const std::string& stamp, uint64_t seed) {
  std::vector<const char*> names;
  for (const std::string& n : wd.names) names.push_back(n.c_str());
  mkdirs(dir);
  CHECK(eg_export_summary_csv(&view, (dir + "/simulation_summary.csv").c_str(), stamp.c_str()));
  CHECK(eg_export_run_details(&world, names.size() == wd.sx.size() ? names.data() : nullptr, &view, dir.c_str(), seed));
  return 0;
}

int run_evaluate(const Args& a, const WorldData& wd, const eg_world& world, const eg_plan_set& plans);
int run_sensitivity(const Args& a, const eg_world& world, const eg_plan_set& plans);
int run_refine(const Args& a, const eg_world& world, const eg_plan_set& plans);
