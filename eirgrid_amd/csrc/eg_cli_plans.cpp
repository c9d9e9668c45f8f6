// eg_cli_plans.cpp — the runs of eirgrid-hip over given plans, none of which trains: --evaluate, --sensitivity and --refine.  Each validates
// what it was given, opens its session (eg_cli.h: policy, then context), runs on the device and writes one directory
// <checkpoint-dir>/<stamp>/<plans|sensitivity|refine>.
#include <algorithm>
#include <cmath>

#include "eg_cli.h"
#include "eg_edit_order.h"

namespace {
const char* const kKind[4] = {"none", "delete", "replace", "insert"};
// the kind, list, year (as a calendar year) and pos columns of an edit's CSV row, a comma behind each
std::string edit_columns(const eg_plan_edit& e) {
  return std::string(kKind[e.kind & 3]) + (e.list ? ",best_deficit_actions," : ",best_actions,") + std::to_string(2025 + int(e.year)) + "," + std::to_string(e.pos) + ",";
}
}  // namespace

// --evaluate: every plan of `plans` scored under one policy (eg_evaluate_plans), plan j as iteration j of the run's seed, --batch plans
// per launch.  <checkpoint-dir>/<stamp>/plans/index.csv gets a row per plan; --top-k K exports the K best plans like top_k/ exports an
// entry (score descending, ties to the lower plan index; failed plans are not ranked).
int run_evaluate(const Args& a, const WorldData& wd, const eg_world& world, const eg_plan_set& plans) {
  Session own;
  if (int rc = own.open(a, world)) return rc;
  const uint32_t n = uint32_t(plans.n_plans);
  // where plan j's entries start in the flat lists
  std::vector<int64_t> pos(n + 1, 0), dpos(n + 1, 0);
  for (uint32_t j = 0; j < n; ++j) {
    int64_t k = 0, dk = 0;
    for (int y = 0; y < EG_YEARS; ++y) { k += plans.best_count[size_t(j) * EG_YEARS + y]; dk += plans.best_deficit_count[size_t(j) * EG_YEARS + y]; }
    pos[j + 1] = pos[j] + k; dpos[j + 1] = dpos[j] + dk;
  }
  auto subset = [&](uint32_t j0, uint32_t m) {      // plans [j0, j0 + m) as a set of their own
    eg_plan_set s = plans;
    s.n_plans = int32_t(m);
    s.best_count = plans.best_count + size_t(j0) * EG_YEARS; s.best_deficit_count = plans.best_deficit_count + size_t(j0) * EG_YEARS;
    s.best_actions = plans.best_actions + pos[j0]; s.best_deficit_actions = plans.best_deficit_actions + dpos[j0];
    s.best_actions_len = pos[j0 + m] - pos[j0]; s.best_deficit_actions_len = dpos[j0 + m] - dpos[j0];
    s.names = plans.names ? plans.names + j0 : nullptr;
    return s;
  };
  std::vector<double> metrics(size_t(n) * 4); std::vector<int32_t> status(n), n_gens(n);
  const auto t0 = Clock::now();
  for (uint32_t j0 = 0; j0 < n; j0 += a.batch) {
    const uint32_t m = std::min(a.batch, n - j0);
    const eg_plan_set s = subset(j0, m);
    eg_episode_out out{}; out.metrics = &metrics[size_t(j0) * 4]; out.status = &status[j0]; out.n_gens = &n_gens[j0];
    CHECK(eg_evaluate_plans(own.ctx, &own.snap, &own.opts, &s, a.seed, j0, &out));
  }
  const double secs = seconds_since(t0);
  std::vector<double> score(n);
  std::vector<uint32_t> order;
  for (uint32_t j = 0; j < n; ++j) {
    score[j] = status[j] == EG_EP_OK ? eg_rank_score(&metrics[size_t(j) * 4], own.mode) : std::nan("");
    if (status[j] == EG_EP_OK) order.push_back(j);
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return score[x] > score[y]; });
  const std::string stamp = time_stamp(kStamp), dir = mkdirs(a.checkpoint_dir + "/" + stamp + "/plans");
  auto name_of = [&](uint32_t j) { return std::string(plans.names && plans.names[j] ? plans.names[j] : ""); };
  {
    std::ofstream f(dir + "/index.csv");
    f << "plan,name,status,score,final_net_emissions,average_public_opinion,total_cost,power_reliability,n_generators\n";
    for (uint32_t j = 0; j < n; ++j) {
      std::string name = name_of(j);      // (a name with a comma, a quote or a line break is quoted, CSV style)
      if (name.find_first_of(",\"\n") != std::string::npos) {
        std::string q = "\"";
        for (char ch : name) { if (ch == '"') q += '"'; q += ch; }
        name = q + "\"";
      }
      f << j << ',' << name << ',' << status[j] << ',' << csv17(&score[j], 1) << ',' << csv17(&metrics[size_t(j) * 4], 4) << ',' << n_gens[j] << '\n';
    }
    if (!f) { std::fprintf(stderr, "error: cannot write %s/index.csv\n", dir.c_str()); return 1; }
  }
  if (a.top_k > 0) {      // the K best plans, each evaluated once more on its own (the same episode: same policy, seed and index)
    Records rec(1); int32_t st = 0;
    for (size_t r = 0; r < order.size() && r < size_t(a.top_k); ++r) {
      const uint32_t j = order[r];
      const eg_plan_set s = subset(j, 1);
      eg_episode_out one = rec.view(); one.status = &st;
      CHECK(eg_evaluate_plans(own.ctx, &own.snap, &own.opts, &s, a.seed, j, &one));
      char sub[24]; std::snprintf(sub, sizeof(sub), "/top_k/%02zu", r + 1);
      if (int rc = export_entry(world, wd, one, dir + sub, stamp, a.seed)) return rc;
    }
  }
  if (order.empty()) std::printf("Evaluated %u plans in %.3f s (%.0f plans/s); no plan finished\n", n, secs, double(n) / std::max(secs, 1e-9));
  else {
    const std::string best = name_of(order[0]).empty() ? std::string() : " (" + name_of(order[0]) + ")";
    std::printf("Evaluated %u plans in %.3f s (%.0f plans/s); best plan %u%s score %.6f; written to %s\n", n, secs, double(n) / std::max(secs, 1e-9),
                order[0], best.c_str(), score[order[0]], dir.c_str());
  }
  return 0;
}

// --sensitivity: the first plan of `plans` as it is and with every one-entry edit of the canonical order (eg_edit_order.h; the order of
// Engine.plan_sensitivity): none; every best_actions entry deleted, in (year, position) order; every best_deficit_actions entry deleted;
// with --sensitivity-replace, every best_actions entry replaced by each listed action.  All variants run as iteration 0 of the run's seed
// (same_index), --batch edits per launch.  <checkpoint-dir>/<stamp>/sensitivity/index.csv gets a row per edit: the calendar year, the
// canonical actions before and after, metrics and score as plans/index.csv writes them, and their differences from row 0 (NaN where
// either variant failed).
int run_sensitivity(const Args& a, const eg_world& world, const eg_plan_set& plans) {
  eg_plan_set base = plans;
  base.n_plans = 1; base.names = nullptr;
  base.best_actions_len = 0; base.best_deficit_actions_len = 0;
  int64_t first[2][EG_YEARS];      // where a year's entries start in the two flat lists
  for (int y = 0; y < EG_YEARS; ++y) {
    first[0][y] = base.best_actions_len; first[1][y] = base.best_deficit_actions_len;
    base.best_actions_len += plans.best_count[y]; base.best_deficit_actions_len += plans.best_deficit_count[y];
  }
  std::vector<eg_plan_edit> edits;
  eg::enumerate_edits(base.best_count, base.best_deficit_count, a.sensitivity_replace.data(), int32_t(a.sensitivity_replace.size()), nullptr, 0, false, edits);
  const uint32_t n = uint32_t(edits.size());
  CHECK(eg_plan_edits_validate(&base, edits.data(), int32_t(n)));
  Session own;
  if (int rc = own.open(a, world)) return rc;
  std::vector<double> metrics(size_t(n) * 4); std::vector<int32_t> status(n);
  const auto t0 = Clock::now();
  for (uint32_t j0 = 0; j0 < n; j0 += a.batch) {
    const uint32_t m = std::min(a.batch, n - j0);
    eg_episode_out out{}; out.metrics = &metrics[size_t(j0) * 4]; out.status = &status[j0];
    CHECK(eg_evaluate_plan_edits(own.ctx, &own.snap, &own.opts, &base, &edits[j0], int32_t(m), a.seed, 0, 1, &out));
  }
  const double secs = seconds_since(t0);
  const std::string dir = mkdirs(a.checkpoint_dir + "/" + time_stamp(kStamp) + "/sensitivity");
  std::vector<double> score(n);
  for (uint32_t j = 0; j < n; ++j) score[j] = status[j] == EG_EP_OK ? eg_rank_score(&metrics[size_t(j) * 4], own.mode) : std::nan("");
  {
    std::ofstream f(dir + "/index.csv");
    f << "edit,kind,list,year,pos,action_before,action_after,status,net_emissions,public_opinion,total_cost,power_reliability,score,"
         "d_net_emissions,d_public_opinion,d_total_cost,d_score\n";
    const bool base_ok = status[0] == EG_EP_OK;
    for (uint32_t j = 0; j < n; ++j) {
      const eg_plan_edit& e = edits[j];
      const double* m = &metrics[size_t(j) * 4];
      f << j << ',';
      if (e.kind == EG_EDIT_NONE) f << "none,,,,,,";
      else {
        const uint8_t* flat = e.list ? base.best_deficit_actions : base.best_actions;
        f << edit_columns(e) << int(flat[first[e.list][e.year] + e.pos]) << ',';
        if (e.kind != EG_EDIT_DELETE) f << int(e.action);
        f << ',';
      }
      const bool both = base_ok && status[j] == EG_EP_OK;
      const double nan = std::nan("");
      const double row[9] = {m[0], m[1], m[2], m[3], score[j], both ? m[0] - metrics[0] : nan, both ? m[1] - metrics[1] : nan, both ? m[2] - metrics[2] : nan,
                             both ? score[j] - score[0] : nan};
      f << status[j] << ',' << csv17(row, 9) << '\n';
    }
    if (!f) { std::fprintf(stderr, "error: cannot write %s/index.csv\n", dir.c_str()); return 1; }
  }
  std::printf("Evaluated %u edits in %.3f s (%.0f edits/s); written to %s\n", n, secs, double(n) / std::max(secs, 1e-9), dir.c_str());
  return 0;
}

// --refine: the plan of `plans` improved greedily on the device (include/eirgrid_hip.h eg_refine_plan): per round every one-entry edit —
// the deletes, with --refine-replace the replaces, with --refine-append the appends — as iteration 0 of the run's seed, the best one
// applied while it improves the score.  <checkpoint-dir>/<stamp>/refine/trajectory.csv: row 0 the start, then a row per applied edit
// (the round, the edit with its calendar year, its place among the round's variants, how many of them failed, score and metrics as
// plans/index.csv writes them), a last line with the stop reason; refine/refined.jsonl: the refined plan, as --evaluate reads it.
int run_refine(const Args& a, const eg_world& world, const eg_plan_set& plans) {
  eg_refine_opts ro{a.cost_only ? 2 : 1, a.refine_rounds, int32_t(a.refine_replace.size()), a.refine_replace.empty() ? nullptr : a.refine_replace.data(),
                    int32_t(a.refine_append.size()), a.refine_append.empty() ? nullptr : a.refine_append.data()};
  CHECK(eg_refine_validate(&plans, &ro));
  Session own;      // (own.plans: the refined plan)
  if (int rc = own.open(a, world)) return rc;
  std::vector<eg_refine_step> steps(size_t(a.refine_rounds));
  int32_t n_steps = 0, stop = 0; double start = 0.0;
  const auto t0 = Clock::now();
  CHECK(eg_refine_plan(own.ctx, &own.snap, &own.opts, &plans, &ro, a.seed, 0, &own.plans, steps.data(), &n_steps, &stop, &start, nullptr));
  const double secs = seconds_since(t0);
  const std::string dir = mkdirs(a.checkpoint_dir + "/" + time_stamp(kStamp) + "/refine");
  static const char* kStop[3] = {"local_optimum", "max_rounds", "base_failed"};
  {
    std::ofstream f(dir + "/trajectory.csv");
    f << "round,kind,list,year,pos,action,variant,n_variants,n_failed,score,net_emissions,public_opinion,total_cost,power_reliability\n";
    f << "start,none,,,,,0,,," << csv17(&start, 1) << ",,,,\n";
    for (int32_t r = 0; r < n_steps; ++r) {
      const eg_refine_step& st = steps[size_t(r)];
      f << r << ',' << edit_columns(st.edit);
      if (st.edit.kind != EG_EDIT_DELETE) f << int(st.edit.action);
      f << ',' << st.variant << ',' << st.n_variants << ',' << st.n_failed << ',' << csv17(&st.score, 1) << ',' << csv17(st.metrics, 4) << '\n';
    }
    f << "# stop: " << kStop[stop] << " after " << n_steps << " steps\n";
    if (!f) { std::fprintf(stderr, "error: cannot write %s/trajectory.csv\n", dir.c_str()); return 1; }
  }
  CHECK(eg_plans_save(own.plans, (dir + "/refined.jsonl").c_str()));
  std::printf("Refined the plan in %d steps (%.3f s): score %.6f -> %.6f, stop: %s; written to %s\n", n_steps, secs, start,
              n_steps > 0 ? steps[size_t(n_steps) - 1].score : start, kStop[stop], dir.c_str());
  return 0;
}
