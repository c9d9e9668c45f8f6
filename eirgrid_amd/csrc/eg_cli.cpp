// eirgrid-hip — command-line training driver on top of libeirgrid_hip.so.
//
// Reproduces the *contract* of the reference driver, not its code: the 18 flags of cli/cli.rs:5-59 with the same names
// and defaults, the data files initialize_map reads (main.rs:74-193), the run-directory / checkpoint layout of
// run_multi_simulation (core/multi_simulation.rs:160-165, :210-290, :396-404, :544-567, :1160-1164) and its schedule
// (replay of the best strategy in "full" runs: the last 10 % of the iterations, or always when the location cache is
// absent, :38-39, :437-465).  Iterations run on the GPU in batches that share one weights snapshot — the GPU
// counterpart of rayon workers cloning the shared weights (:457-460) — and are folded into the weights either one by
// one in index order (--update sequential: multi_simulation.rs:494-508 verbatim) or with the batch form
// (--update reduced, default).  The best-run CSV export (--enable-csv-export, N3) writes what the
// reference's exporter writes: simulation_summary.csv, improvement_history.csv, yearly_details/{settlements,generators,
// carbon_offsets}.csv and operation_logs/generator_operation_logs.csv (csrc/eg_export.cpp describes their contents).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <random>

#include <dirent.h>

#include "eg_cli.h"
#include "eg_json.h"

namespace {

void usage() {
  std::puts("Usage: eirgrid-hip [OPTIONS]\n"
            "  -n, --iterations <N>            [default: 1000]\n  -p, --parallel\n      --no-continue\n"
            "  -c, --checkpoint-dir <DIR>      [default: checkpoints]\n  -i, --checkpoint-interval <N>   [default: 5]\n"
            "  -r, --progress-interval <SECS>  [default: 10]\n  -C, --cache-dir <DIR>           [default: cache]\n"
            "      --force-full-simulation\n      --enable-timing\n      --seed <SEED>\n  -v, --verbose-state-logging\n"
            "      --cost-only\n      --enable-energy-sales\n      --enable-csv-export\n      --debug-logging\n      --debug-weights\n"
            "      --enable-construction-delays\n      --track-weight-history\n"
            "engine options:\n      --world <FILE>       world in eirgrid_amd JSON form (default: read <assets-dir> like the reference)\n"
            "      --assets-dir <DIR>   settlements.json, ireland_generators.csv, coastline_points.json [default: aiSimulator/assets]\n"
            "      --batch <B>          iterations per GPU launch [default: 1024]\n      --update <sequential|reduced>  [default: reduced]\n"
            "      --device <N>         [default: 0]\n"
            "      --gpus <N>           train on devices 0..N-1, one rank each (--batch stays the global iterations per update)\n"
            "      --devices <LIST>     train on these devices, one rank each, e.g. 0,1 (repeats: ranks sharing a GPU)\n"
            "      --existing-operational-at-start\n"
            "      --stop-after <N>     stop like an interrupted run once N iterations are done and checkpointed (resume tests)\n"
            "      --dump-world <FILE>  write the world as loaded (the --world JSON form) and exit; needs no GPU\n"
            "      --no-replay-hoist    run every replay iteration of a batch on its own (default: the replay iterations of a batch —\n"
            "                           one and the same computation — are computed once; identical results either way)\n"
            "      --top-k <K>          keep the K best distinct scenarios of the run (0..64, ranked by score_metrics in the run's mode)\n"
            "                           and write them to enhanced_csv/<stamp>/top_k/ [default: 0 = off]\n"
            "      --evaluate <FILE>    score the plans of FILE (a checkpoint, or JSON Lines of best_actions / best_deficit_actions with an\n"
            "                           optional name) and exit: plan j replays as iteration j of --seed [default 0], --batch plans per\n"
            "                           launch; writes <checkpoint-dir>/<stamp>/plans/index.csv, with --top-k K also the K best plans'\n"
            "                           exports in plans/top_k/; no training runs\n"
            "      --evaluate-policy <CKPT>  the policy the plans (or the edits of --sensitivity) are evaluated under [default: a fresh one]\n"
            "      --sensitivity <FILE> which actions of a plan matter: the first plan of FILE (as --evaluate reads it) is scored as it is and\n"
            "                           with every entry of its two lists deleted in turn, all as iteration 0 of --seed [default 0] on one\n"
            "                           device; writes <checkpoint-dir>/<stamp>/sensitivity/index.csv (metrics, score and their\n"
            "                           differences from the unedited plan, one row per edit) and exits; no training runs\n"
            "      --sensitivity-replace <a,b,...>  also every best_actions entry replaced by each of these canonical actions (0..60)\n"
            "      --refine <FILE>      improve a plan greedily: FILE holds one plan (as --evaluate reads it); round after round every one-entry\n"
            "                           edit of it is scored as iteration 0 of --seed [default 0] on one device and the best one applied, until\n"
            "                           none improves the score (--cost-only: the cost score); writes <checkpoint-dir>/<stamp>/refine/\n"
            "                           trajectory.csv (a row per applied edit) and refined.jsonl (the plan, for --evaluate) and exits\n"
            "      --refine-rounds <N>  apply at most N edits [default: 64]\n"
            "      --refine-replace <a,b,...>  besides deleting an entry, try it replaced by each of these canonical actions (0..60)\n"
            "      --refine-append <a,b,...>   ... and each of these actions appended to each year's best_actions list");
}

// digits only, at most max_digits of them, lo <= value <= hi: every number of the command line that is checked at all
bool parse_uint(const std::string& text, size_t max_digits, int lo, int hi, int32_t* out) {
  if (text.empty() || text.size() > max_digits || text.find_first_not_of("0123456789") != std::string::npos) return false;
  *out = std::atoi(text.c_str());
  return *out >= lo && *out <= hi;
}
// a comma-separated list of such numbers, appended to `out`; an empty item is refused
template <class T> bool parse_list(const std::string& list, size_t max_digits, int hi, std::vector<T>& out) {
  for (size_t pos = 0; pos <= list.size();) {
    const size_t comma = std::min(list.find(',', pos), list.size());
    int32_t k;
    if (!parse_uint(list.substr(pos, comma - pos), max_digits, 0, hi, &k)) return false;
    out.push_back(T(k));
    pos = comma + 1;
  }
  return true;
}

bool parse(int argc, char** argv, Args& a) {
  auto need = [&](int& i) -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "error: %s needs a value\n", argv[i]); std::exit(2); } return argv[++i]; };
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i], val;
    const size_t eq = s.find('=');
    bool has_val = false;
    if (s.rfind("--", 0) == 0 && eq != std::string::npos) { val = s.substr(eq + 1); s = s.substr(0, eq); has_val = true; }
    auto v = [&]() -> std::string { return has_val ? val : std::string(need(i)); };
    if (s == "-n" || s == "--iterations") a.iterations = std::strtoull(v().c_str(), nullptr, 10);
    else if (s == "-p" || s == "--parallel") a.parallel = true;
    else if (s == "--no-continue") a.no_continue = true;
    else if (s == "-c" || s == "--checkpoint-dir") a.checkpoint_dir = v();
    else if (s == "-i" || s == "--checkpoint-interval") a.checkpoint_interval = std::max<uint64_t>(1, std::strtoull(v().c_str(), nullptr, 10));
    else if (s == "-r" || s == "--progress-interval") a.progress_interval = std::strtoull(v().c_str(), nullptr, 10);
    else if (s == "-C" || s == "--cache-dir") a.cache_dir = v();
    else if (s == "--force-full-simulation") a.force_full_simulation = true;
    else if (s == "--enable-timing") a.enable_timing = true;
    else if (s == "--seed") { a.seed = std::strtoull(v().c_str(), nullptr, 10); a.has_seed = true; }
    else if (s == "-v" || s == "--verbose-state-logging") a.verbose_state_logging = true;
    else if (s == "--cost-only") a.cost_only = true;
    else if (s == "--enable-energy-sales") a.enable_energy_sales = true;     // SetTrue flags with default true (Q7)
    else if (s == "--enable-csv-export") a.enable_csv_export = true;
    else if (s == "--debug-logging") a.debug_logging = true;
    else if (s == "--debug-weights") a.debug_weights = true;
    else if (s == "--enable-construction-delays") a.enable_construction_delays = true;
    else if (s == "--track-weight-history") a.track_weight_history = true;
    else if (s == "--world") a.world_json = v();
    else if (s == "--assets-dir") a.assets_dir = v();
    else if (s == "--batch") a.batch = uint32_t(std::max<uint64_t>(1, std::strtoull(v().c_str(), nullptr, 10)));
    else if (s == "--update") a.update = v();
    else if (s == "--device") { a.device = std::atoi(v().c_str()); a.device_given = true; }
    else if (s == "--gpus" || s == "--devices") {
      const std::string list = v();
      const bool gpus = s == "--gpus";
      if (a.gpus_given || !a.ranks.empty()) { std::fprintf(stderr, "error: --gpus and --devices are given more than once\n"); return false; }
      a.gpus_given = gpus;
      // --gpus N: a count >= 1; --devices: comma-separated ordinals >= 0 (digits only)
      int32_t k = 0;
      if (gpus ? !parse_uint(list, 6, 0, 999999, &k) : !parse_list(list, 6, 999999, a.ranks)) {
        std::fprintf(stderr, "error: %s needs %s, got '%s'\n", s.c_str(), gpus ? "a number of GPUs" : "a comma-separated list of device numbers", list.c_str());
        return false;
      }
      if (gpus && k < 1) { std::fprintf(stderr, "error: --gpus needs at least 1\n"); return false; }
      for (int32_t d = 0; d < k; ++d) a.ranks.push_back(d);
    }
    else if (s == "--existing-operational-at-start") a.existing_operational_at_start = true;
    else if (s == "--stop-after") a.stop_after = std::strtoull(v().c_str(), nullptr, 10);
    else if (s == "--dump-world") a.dump_world = v();
    else if (s == "--no-replay-hoist") a.replay_hoist = false;
    else if (s == "--top-k") {
      const std::string k = v();
      if (!parse_uint(k, 3, 0, EG_TOPK_MAX, &a.top_k)) { std::fprintf(stderr, "error: --top-k needs a number from 0 to %d, got '%s'\n", EG_TOPK_MAX, k.c_str()); return false; }
    }
    else if (s == "--evaluate") a.evaluate = v();
    else if (s == "--evaluate-policy") a.evaluate_policy = v();
    else if (s == "--sensitivity") a.sensitivity = v();
    else if (s == "--sensitivity-replace" || s == "--refine-replace" || s == "--refine-append") {
      const std::string list = v();
      if (!parse_list(list, 2, EG_N_ACTIONS - 1, s == "--sensitivity-replace" ? a.sensitivity_replace : s == "--refine-replace" ? a.refine_replace : a.refine_append)) {
        std::fprintf(stderr, "error: %s needs a comma-separated list of canonical actions 0..%d, got '%s'\n", s.c_str(), EG_N_ACTIONS - 1, list.c_str());
        return false;
      }
    }
    else if (s == "--refine") a.refine = v();
    else if (s == "--refine-rounds") {
      const std::string k = v();
      a.refine_rounds_given = true;
      if (!parse_uint(k, 6, 1, 999999, &a.refine_rounds)) { std::fprintf(stderr, "error: --refine-rounds needs a number from 1 to 999999, got '%s'\n", k.c_str()); return false; }
    }
    else if (s == "-h" || s == "--help") { usage(); std::exit(0); }
    else { std::fprintf(stderr, "error: unexpected argument '%s'\n", argv[i]); usage(); return false; }
  }
  if (a.update != "sequential" && a.update != "reduced") return false;
  if (!a.ranks.empty() && a.device_given) { std::fprintf(stderr, "error: --device cannot be combined with --gpus / --devices\n"); return false; }
  if (a.ranks.size() > 1 && a.update == "sequential") {
    std::fprintf(stderr, "error: --update sequential folds iterations one by one on one device; with more than one rank use --update reduced\n");
    return false;
  }
  if (a.ranks.size() == 1) a.device = a.ranks[0];      // one rank: the single-device run on that device
  if (!a.evaluate_policy.empty() && a.evaluate.empty() && a.sensitivity.empty() && a.refine.empty()) { std::fprintf(stderr, "error: --evaluate-policy needs --evaluate, --sensitivity or --refine\n"); return false; }
  if (a.refine.empty() && (a.refine_rounds_given || !a.refine_replace.empty() || !a.refine_append.empty())) {
    std::fprintf(stderr, "error: --refine-rounds, --refine-replace and --refine-append need --refine\n"); return false;
  }
  if (!a.refine.empty() && (!a.evaluate.empty() || !a.sensitivity.empty())) { std::fprintf(stderr, "error: --refine, --sensitivity and --evaluate are separate runs\n"); return false; }
  if (!a.refine.empty() && a.ranks.size() > 1) { std::fprintf(stderr, "error: --refine runs on one device (no --gpus / --devices)\n"); return false; }
  if (!a.sensitivity_replace.empty() && a.sensitivity.empty()) { std::fprintf(stderr, "error: --sensitivity-replace needs --sensitivity\n"); return false; }
  if (!a.sensitivity.empty() && !a.evaluate.empty()) { std::fprintf(stderr, "error: --sensitivity and --evaluate are separate runs\n"); return false; }
  if (!a.sensitivity.empty() && a.ranks.size() > 1) { std::fprintf(stderr, "error: --sensitivity runs on one device (no --gpus / --devices)\n"); return false; }
  if (!a.evaluate.empty() && a.ranks.size() > 1) { std::fprintf(stderr, "error: --evaluate runs on one device (no --gpus / --devices)\n"); return false; }
  return true;
}

bool parse_json(const std::string& path, eg::Json& root) {
  std::string text; if (!read_file(path, text)) return false;
  eg::JsonParser ps{text.data(), text.data() + text.size(), {}};
  return ps.value(root);
}
void nums(const eg::Json* j, std::vector<double>& out) { if (j && j->kind == eg::Json::Arr) for (auto& v : j->arr) out.push_back(v.num); }

bool load_world_json(const std::string& path, WorldData& w) {   // eirgrid_amd.world.World.to_json_dict
  eg::Json r; if (!parse_json(path, r) || r.kind != eg::Json::Obj) return false;
  std::vector<double> pop, type;
  nums(r.get("settlement_x"), w.sx); nums(r.get("settlement_y"), w.sy); nums(r.get("settlement_pop"), pop);
  nums(r.get("existing_x"), w.gx); nums(r.get("existing_y"), w.gy); nums(r.get("existing_type"), type); nums(r.get("existing_capacity"), w.gcap);
  nums(r.get("coast_x"), w.cx); nums(r.get("coast_y"), w.cy);
  for (double p : pop) w.spop.push_back(uint32_t(p));
  for (double t : type) w.gtype.push_back(int32_t(t));
  if (const eg::Json* nm = r.get("settlement_names"); nm && nm->kind == eg::Json::Arr && nm->arr.size() == w.sx.size())
    for (auto& v : nm->arr) w.names.push_back(v.str);
  return !w.sx.empty() && w.sx.size() == w.sy.size() && w.sx.size() == w.spop.size() && w.gx.size() == w.gtype.size();
}
// const_funcs.rs:124-136 + constants.rs:131-134, :270-271
bool lat_lon_to_grid(double lat, double lon, double& x, double& y) {
  if (lat < 51.4 || lat > 55.4 || lon < -10.6 || lon > -5.9) return false;
  x = (lon - -10.6) * 10638.297872340427; y = (lat - 51.4) * 12500.0;
  x = std::min(std::max(x, 0.0), 50000.0); y = std::min(std::max(y, 0.0), 50000.0);
  return true;
}
bool load_reference_assets(const std::string& dir, WorldData& w) {   // main.rs:74-193
  eg::Json s;
  if (!parse_json(dir + "/settlements.json", s)) return false;
  const eg::Json* list = s.get("settlements");
  if (!list || list->kind != eg::Json::Arr) return false;
  for (auto& e : list->arr) {   // data/settlements_loader.rs:23-41
    const eg::Json *lat = e.get("lat"), *lon = e.get("lon"), *pop = e.get("population");
    double x, y;
    if (lat && lon && pop && lat_lon_to_grid(lat->num, lon->num, x, y)) {
      w.sx.push_back(x); w.sy.push_back(y); w.spop.push_back(uint32_t(pop->num));
      const eg::Json* name = e.get("name"); w.names.push_back(name ? name->str : "Settlement_" + std::to_string(w.names.size()));
    }
  }
  std::string csv;
  if (!read_file(dir + "/ireland_generators.csv", csv)) return false;
  std::istringstream in(csv); std::string line; bool header = true;
  while (std::getline(in, line)) {   // data/generators_loader.rs:133-206
    if (header) { header = false; continue; }
    if (line.empty()) continue;
    std::vector<std::string> col; std::stringstream ls(line); std::string c;
    while (std::getline(ls, c, ',')) col.push_back(c);
    if (col.size() < 4) continue;
    std::string fuel = col[3]; while (!fuel.empty() && (fuel.back() == '\r' || fuel.back() == ' ')) fuel.pop_back();
    std::transform(fuel.begin(), fuel.end(), fuel.begin(), ::tolower);
    int t = fuel == "gas" ? 7 : fuel == "coal" ? 6 : fuel == "wind" ? 0 : fuel == "hydro" ? 10 : fuel == "oil" ? 8 : fuel == "biomass" ? 9 : -1;
    if (t < 0) { std::fprintf(stderr, "Invalid fuel type: %s\n", col[3].c_str()); return false; }
    double lat = std::min(std::max(std::atof(col[1].c_str()), 51.4), 55.4), lon = std::min(std::max(std::atof(col[2].c_str()), -10.6), -5.9), x, y;
    lat_lon_to_grid(lat, lon, x, y);
    w.gx.push_back(x); w.gy.push_back(y); w.gtype.push_back(t); w.gcap.push_back(std::atof(col[0].c_str()));
  }
  eg::Json cst;
  if (parse_json(dir + "/coastline_points.json", cst))
    if (const eg::Json* g = cst.get("grid_coords"); g && g->kind == eg::Json::Arr)
      for (auto& pt : g->arr) if (pt.kind == eg::Json::Arr && pt.arr.size() >= 2) { w.cx.push_back(pt.arr[0].num); w.cy.push_back(pt.arr[1].num); }
  return !w.sx.empty();
}

std::string newest_run_dir(const std::string& base) {   // multi_simulation.rs:217-235: 15-character names, year <= 2025
  std::string best;
  if (DIR* d = ::opendir(base.c_str())) {
    while (dirent* e = ::readdir(d)) {
      std::string n = e->d_name;
      if (n.size() != 15 || n[8] != '_') continue;
      if (std::atoi(n.substr(0, 4).c_str()) > 2025) continue;
      if (!exists(base + "/" + n + "/latest_weights.json")) continue;
      if (n > best) best = n;
    }
    ::closedir(d);
  }
  return best.empty() ? best : base + "/" + best;
}

int load_world(const Args& a, WorldData& wd) {      // --world, or the reference's assets; what was loaded goes to stdout
  if (!a.world_json.empty()) { if (!load_world_json(a.world_json, wd)) { std::fprintf(stderr, "error: cannot read world %s\n", a.world_json.c_str()); return 1; } }
  else if (!load_reference_assets(a.assets_dir, wd)) { std::fprintf(stderr, "error: cannot read %s/{settlements.json,ireland_generators.csv} (use --world or --assets-dir)\n", a.assets_dir.c_str()); return 1; }
  std::printf("World: %zu settlements, %zu existing generators, %zu coastline points\n", wd.sx.size(), wd.gx.size(), wd.cx.size());
  // the fuel mix as data/generators_loader.rs:47-57 maps it (gas -> GasCombinedCycle, oil -> GasPeaker, ...)
  static const char* kTypeName[EG_N_TYPES] = {"OnshoreWind", "OffshoreWind", "DomesticSolar", "CommercialSolar", "UtilitySolar", "Nuclear", "CoalPlant",
                                              "GasCombinedCycle", "GasPeaker", "Biomass", "HydroDam", "PumpedStorage", "BatteryStorage", "TidalGenerator", "WaveEnergy"};
  int count[EG_N_TYPES] = {0};
  for (int32_t t : wd.gtype) if (t >= 0 && t < EG_N_TYPES) count[t] += 1;
  std::string mix;
  for (int t = 0; t < EG_N_TYPES; ++t) if (count[t]) mix += (mix.empty() ? "" : ", ") + std::string(kTypeName[t]) + " " + std::to_string(count[t]);
  std::printf("Existing generators by type: %s\n", mix.c_str());
  return 0;
}

int dump_world(const Args& a, const WorldData& wd) {      // --dump-world: the world as loaded, in the --world JSON form
  std::ofstream f(a.dump_world);
  if (!f) { std::fprintf(stderr, "error: cannot write %s\n", a.dump_world.c_str()); return 1; }
  auto arr = [&](const char* key, const std::vector<double>& v) { f << "\"" << key << "\": [" << csv17(v.data(), int(v.size()), ", ") << "], "; };
  f << "{";
  arr("settlement_x", wd.sx); arr("settlement_y", wd.sy); arr("settlement_pop", std::vector<double>(wd.spop.begin(), wd.spop.end()));
  arr("existing_x", wd.gx); arr("existing_y", wd.gy); arr("existing_type", std::vector<double>(wd.gtype.begin(), wd.gtype.end()));
  arr("existing_capacity", wd.gcap); arr("coast_x", wd.cx); arr("coast_y", wd.cy);
  f << "\"existing_operational_at_start\": " << (a.existing_operational_at_start ? "true" : "false") << "}\n";
  std::printf("World written to %s\n", a.dump_world.c_str());
  return 0;
}

// The training run: --iterations iterations in batches on one device or, with more than one rank, the same reduced-update loop on an
// eg_group (the exchange between the ranks is inside the library); checkpoints, progress lines and the best run's export as the header says.
int run_training(Args& a, const WorldData& wd, const eg_world& world) {
  Session own;
  eg_ctx*& ctx = own.ctx; eg_group*& group = own.group; eg_policy*& policy = own.policy;
  if (a.gpus_given && int32_t(a.ranks.size()) > eg_device_count()) {
    std::fprintf(stderr, "error: --gpus %zu: only %d device(s) visible\n", a.ranks.size(), eg_device_count()); return 2;
  }
  if (a.ranks.size() > 1) {
    group = eg_group_create(a.ranks.data(), int32_t(a.ranks.size()), &world);
    if (!group) { std::fprintf(stderr, "eg_group_create: %s\n", eg_last_error()); return 1; }
    std::printf("Ranks: %zu on devices", a.ranks.size());
    for (int32_t d : a.ranks) std::printf(" %d", d);
    std::printf(" (%u iterations per update, sharded)\n", a.batch);
  } else if (int rc = own.create(a, world)) return rc;
  // The reference's replay phases (the last 10 % of a run, --force-full-simulation: core/multi_simulation.rs:38-39, :437-465) run the
  // same replay in every iteration of a batch: computed once unless asked otherwise (worlds the hoist is not sized for: every
  // iteration on its own, silently — the results are the same)
  if (a.replay_hoist) (void)(group ? eg_group_replay_hoist(group, 1) : eg_replay_hoist(ctx, 1));

  // run directory and resume (multi_simulation.rs:160-165, :210-290, :396-404)
  uint64_t start_iteration = 0; std::string run_dir;
  if (!a.no_continue) {
    run_dir = newest_run_dir(a.checkpoint_dir);
    if (!run_dir.empty()) {
      policy = eg_policy_load_json((run_dir + "/latest_weights.json").c_str());
      if (policy) {
        std::string it; if (read_file(run_dir + "/checkpoint_iteration.txt", it)) start_iteration = std::strtoull(it.c_str(), nullptr, 10);
        std::printf("Loaded weights from %s (iteration %llu)\n", run_dir.c_str(), (unsigned long long)start_iteration);
      } else { std::fprintf(stderr, "warning: %s\n", eg_last_error()); run_dir.clear(); }
    }
  }
  if (!policy) policy = eg_policy_new();
  if (run_dir.empty()) run_dir = a.checkpoint_dir + "/2024" + time_stamp("%m%d_%H%M%S");   // the literal "2024" of multi_simulation.rs:162 (Q17)
  mkdirs(run_dir);
  if (!a.has_seed) { std::random_device rd; a.seed = (uint64_t(rd()) << 32) | rd(); }
  const bool cache_loaded = exists(a.cache_dir + "/location_analysis.json");   // multi_simulation.rs:150-154
  std::printf("Starting multi-simulation optimization with %llu iterations (%llu completed, %llu remaining) in directory %s\n",
              (unsigned long long)a.iterations, (unsigned long long)start_iteration,
              (unsigned long long)(a.iterations > start_iteration ? a.iterations - start_iteration : 0), run_dir.c_str());

  // The run that is summarised and exported at the end: the reference's `best_result`, a fold over this process's iterations in
  // iteration order that starts at None (core/multi_simulation.rs:384, :613-620; --cost-only reaches it as optimization_mode).
  // The library folds every batch on the device behind its rollout (eg_best_result_track) and keeps the held run's record.
  Records best_run(1);
  std::vector<uint8_t> mask;
  std::vector<double> metrics; std::vector<int32_t> n_run, n_def; std::vector<uint8_t> run_log, def_log;
  eg_opts opts{a.enable_energy_sales ? 1 : 0, 0, a.enable_csv_export ? 1 : 0};   // the export needs the best episode's yearly rows
  const uint64_t final_full = a.iterations * 10 / 100;   // FULL_RUN_PERCENTAGE, multi_simulation.rs:38, :437
  const auto t0 = Clock::now(); auto last_progress = t0;
  uint64_t done = start_iteration, last_checkpoint = start_iteration / a.checkpoint_interval;
  const bool reduced = a.update == "reduced";
  unsigned failed_sequential = 0;      // --update sequential: episodes that did not finish (reduced mode counts them on the device)
  // reduced mode keeps the policy on the device: pushed once, every batch is enqueued without a host round trip and the
  // host copy is refreshed (eg_policy_pull) when a checkpoint or a progress line needs it
  if (reduced) CHECK(group ? eg_group_push(group, policy, &opts) : eg_policy_push(ctx, policy, &opts));
  CHECK(group ? eg_group_best_result_track(group, a.cost_only ? 2 : 1) : eg_best_result_track(ctx, a.cost_only ? 2 : 1));
  // --top-k: the K best distinct scenarios of this process's iterations, ranked in the run's mode, kept on the device behind every batch
  if (a.top_k > 0) CHECK(group ? eg_group_top_k_track(group, a.top_k, a.cost_only ? 2 : 1) : eg_top_k_track(ctx, a.top_k, a.cost_only ? 2 : 1));
  const uint64_t full_from = a.iterations - std::min(a.iterations, final_full);   // multi_simulation.rs:437-465
  while (done < a.iterations) {
    uint32_t n = uint32_t(std::min<uint64_t>(a.batch, a.iterations - done));
    const bool always_full = a.force_full_simulation || !cache_loaded;
    if (reduced) {
      if (!always_full && done < full_from && done + n > full_from) n = uint32_t(full_from - done);   // a batch never straddles the switch
      const bool full = always_full || done >= full_from;
      if (group) CHECK(eg_group_step(group, a.seed, done, n, full ? 1u : 0u, a.seed + done));
      else CHECK(eg_device_step(ctx, a.seed, done, n, full ? 1u : 0u, a.seed + done));   // replay (once a best strategy exists) when full
    } else {
      eg_policy_snapshot snap; CHECK(eg_policy_snapshot_view(policy, &snap));
      CHECK(eg_upload_snapshot(ctx, &snap, &opts));
      mask.assign(n, 0);
      for (uint32_t i = 0; i < n; ++i) {
        const bool full = always_full || done + i >= full_from;
        mask[i] = (full && snap.has_best && snap.best_count) ? 1 : 0;
      }
      metrics.resize(size_t(n) * 4); n_run.resize(size_t(n) * EG_YEARS); n_def.resize(size_t(n) * EG_YEARS);
      run_log.resize(size_t(n) * EG_RUN_CAP); def_log.resize(size_t(n) * EG_DEF_CAP);
      std::vector<int32_t> status(n);
      eg_episode_out out{}; out.metrics = metrics.data(); out.n_run = n_run.data(); out.n_def = n_def.data(); out.run_log = run_log.data();
      out.def_log = def_log.data(); out.status = status.data();
      CHECK(eg_rollout_launch(ctx, a.seed, done, n, mask.data()));
      CHECK(eg_fetch(ctx, &out));
      for (uint32_t i = 0; i < n; ++i)   // multi_simulation.rs:494-508, in iteration order
        if (status[i] != EG_EP_OK) failed_sequential += 1;
        else
          CHECK(eg_policy_apply_episode(policy, &metrics[size_t(i) * 4], &n_run[size_t(i) * EG_YEARS], &run_log[size_t(i) * EG_RUN_CAP],
                                        &n_def[size_t(i) * EG_YEARS], &def_log[size_t(i) * EG_DEF_CAP], a.seed + done + i));
    }
    done += n;
    const auto now = Clock::now();
    const bool checkpoint_due = done / a.checkpoint_interval != last_checkpoint || done == a.iterations;
    const bool progress_due = std::chrono::duration<double>(now - last_progress).count() >= double(a.progress_interval) || done == a.iterations;
    if (reduced && (checkpoint_due || progress_due)) CHECK(group ? eg_group_pull(group, 0, policy) : eg_policy_pull(ctx, policy));
    if (checkpoint_due) {   // multi_simulation.rs:544-567
      last_checkpoint = done / a.checkpoint_interval;
      CHECK(eg_policy_save_json(policy, (run_dir + "/thread_0_weights.json").c_str()));
      CHECK(eg_policy_save_json(policy, (run_dir + "/latest_weights.json").c_str()));
      if (a.track_weight_history) CHECK(eg_policy_append_weight_history(policy, (run_dir + "/weight_history.json").c_str(), done - 1));   // :557-560
      std::ofstream(run_dir + "/checkpoint_iteration.txt") << done;
    }
    if (progress_due) {   // :303-382
      last_progress = now;
      const double secs = std::chrono::duration<double>(now - t0).count();
      double bm[4] = {eg_policy_get_scalar(policy, 5), eg_policy_get_scalar(policy, 6), eg_policy_get_scalar(policy, 7), eg_policy_get_scalar(policy, 8)};
      // (failed: episodes that ran out of the per-episode capacities — replay-doubled lists; they are not part of
      //  iteration_count and never silently dropped from the count)
      std::printf("Progress: %llu/%llu iterations (%.1f%%), %.0f iterations/s | best score %.6f (emissions %.1f t, cost EUR %.2fB, opinion %.1f%%), %u without improvement, %u episodes failed\n",
                  (unsigned long long)done, (unsigned long long)a.iterations, 100.0 * double(done) / double(a.iterations),
                  double(done - start_iteration) / std::max(secs, 1e-9), eg_policy_get_scalar(policy, 4) != 0.0 ? eg_score_metrics(bm, a.cost_only ? 1 : 0) : 0.0,
                  bm[0], bm[2] / 1e9, bm[1] * 100.0, unsigned(eg_policy_get_scalar(policy, 2)), unsigned(eg_policy_get_scalar(policy, 13)) + failed_sequential);
      std::fflush(stdout);
    }
    if (a.stop_after && done >= a.stop_after && done < a.iterations) {
      if (!checkpoint_due) { std::fprintf(stderr, "error: --stop-after needs a checkpoint at the stop (use -i 1 or a divisor)\n"); return 2; }
      std::printf("Stopped after %llu iterations (--stop-after); resume with the same command\n", (unsigned long long)done);
      return 0;
    }
  }
  CHECK(eg_policy_save_json(policy, (run_dir + "/best_weights.json").c_str()));   // multi_simulation.rs:1160-1164
  std::string stamp, dir;
  if (a.enable_csv_export || a.top_k > 0) {   // multi_simulation.rs:852-859, :912-921; csv_export.rs:114-127 (directory named after the time of export)
    stamp = time_stamp(kStamp);
    dir = mkdirs(run_dir + "/enhanced_csv/" + stamp);
  }
  if (a.enable_csv_export) CHECK(eg_policy_export_improvement_csv(policy, (dir + "/improvement_history.csv").c_str()));
  int64_t best_index = -1; int32_t state = 0;      // (state 1: an iteration finished and its record is held)
  eg_episode_out best_view = best_run.view();
  CHECK(group ? eg_group_fetch_best_result(group, &best_view, &state, &best_index) : eg_fetch_best_result(ctx, &best_view, &state, &best_index));
  if (state == 1) {   // multi_simulation.rs:821-850
    const double* bm = best_run.metrics.data();
    std::printf("BEST SIMULATION RESULTS SUMMARY (iteration %lld)\nFinal net emissions: %.2f tonnes\nEmissions Status: %s\nAverage public opinion: %.1f%%\n"
                "Total cost: EUR %.2f billion accumulated\nPower reliability: %.1f%%\n", (long long)best_index, bm[0],
                bm[0] <= 0.0 ? "NET ZERO ACHIEVED" : "NET ZERO NOT ACHIEVED", bm[1] * 100.0, bm[2] / 1e9, bm[3] * 100.0);
  }
  if (a.enable_csv_export) {
    if (state == 1) { if (int rc = export_entry(world, wd, best_view, dir, stamp, a.seed)) return rc; }
    else std::puts("note: no iteration finished in this run; simulation_summary.csv and the detail files not written");
  }
  if (a.top_k > 0) {      // top_k/index.csv: rank, score, iteration, metrics; with the CSV export one directory per entry, like the best run's
    Records top(size_t(a.top_k));
    std::vector<double> score_k(size_t(a.top_k)); std::vector<int64_t> index_k(size_t(a.top_k));
    eg_episode_out out = top.view(); int32_t held = 0;
    CHECK(group ? eg_group_fetch_top_k(group, &out, &held, score_k.data(), index_k.data()) : eg_fetch_top_k(ctx, &out, &held, score_k.data(), index_k.data()));
    const std::string tk = mkdirs(dir + "/top_k");
    std::ofstream f(tk + "/index.csv");
    f << "rank,score,iteration,final_net_emissions,average_public_opinion,total_cost,power_reliability\n";
    for (int32_t r = 0; r < held; ++r) {
      f << r + 1 << ',' << csv17(&score_k[size_t(r)], 1) << ',' << index_k[size_t(r)] << ',' << csv17(&top.metrics[size_t(r) * 4], 4) << '\n';
      if (!a.enable_csv_export) continue;
      char sub[16]; std::snprintf(sub, sizeof(sub), "/%02d", r + 1);
      if (int rc = export_entry(world, wd, top.view(size_t(r)), tk + sub, stamp, a.seed)) return rc;
    }
    if (!f) { std::fprintf(stderr, "error: cannot write %s/index.csv\n", tk.c_str()); return 1; }
    std::printf("Top %d distinct scenarios (%d held) written to %s\n", a.top_k, held, tk.c_str());
  }
  std::printf("Done: %llu iterations in %s (%u episodes failed); best_weights.json, latest_weights.json, checkpoint_iteration.txt written\n",
              (unsigned long long)done, run_dir.c_str(), unsigned(eg_policy_get_scalar(policy, 13)) + failed_sequential);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  Args a;
  if (!parse(argc, argv, a)) return 2;
  std::puts("EirGrid Power System Simulator (2025-2050) — MI355X rollout engine");
  Session loaded;      // the plans of --evaluate, --sensitivity or --refine (they read their file the same way): every invalid line is reported before a device is touched
  const std::string& plans_file = !a.evaluate.empty() ? a.evaluate : !a.sensitivity.empty() ? a.sensitivity : a.refine;
  if (!plans_file.empty() && !(loaded.plans = eg_plans_load(plans_file.c_str()))) { std::fprintf(stderr, "error: %s\n", eg_last_error()); return 1; }
  if (!a.refine.empty() && loaded.plans->n_plans != 1) { std::fprintf(stderr, "error: --refine needs a file with one plan, %s holds %d\n", a.refine.c_str(), loaded.plans->n_plans); return 2; }
  if (a.enable_construction_delays) { std::fprintf(stderr, "error: --enable-construction-delays is not implemented on the device (DESIGN.md §6)\n"); return 2; }
  WorldData wd;
  if (int rc = load_world(a, wd)) return rc;
  if (!a.dump_world.empty()) return dump_world(a, wd);
  const eg_world world = wd.view(a.existing_operational_at_start);
  if (!loaded.plans) return run_training(a, wd, world);
  if (!a.refine.empty()) return run_refine(a, world, *loaded.plans);
  return a.sensitivity.empty() ? run_evaluate(a, wd, world, *loaded.plans) : run_sensitivity(a, world, *loaded.plans);
}
