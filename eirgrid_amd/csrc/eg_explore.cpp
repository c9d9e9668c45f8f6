// eg_explore.cpp — eg_explore_plans: a Pareto local search over one-entry edits and moves of the plans of a front (include/eirgrid_hip.h),
// its validator and eg_explore_neighbourhood.  The archive lives on the device across the generations of a call, in eg_breed_plans'
// buffer (eg_internal.h breed_at); the host keeps, per member of the current frontier, its number and the per-year counts of its two
// lists, enumerates a generation CHUNK BY CHUNK from them (one member's neighbourhood at a time: a generation's variants are never
// held), uploads 12 bytes a variant and the routing, and reads one buffer back per generation with a row per new member
// (eg_breed.h k_breed_gather, eg_explore.h k_explore_turnover).  The packing, the launch of a chunk, the archive and the shared option
// checks are eg_plan_host.cpp's.
#include <algorithm>
#include <cstring>

#include "eg_edit_order.h"
#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_explore_opts) == 64 && sizeof(eg_explore_generation) == 40 && sizeof(eg_explore_member) == 88, "the explore structs are part of the C ABI");
static_assert(EG_CROSS_MAX_VARIANTS <= EG_PARETO_MAX * 64, "k_breed_gather counts a chunk's valid variants with one wave per entry");

namespace {
const char* const kFn = "eg_explore_plans";

// a plan as the host follows it: its number and the per-year lengths of its two lists
struct Base {
  int64_t number = 0;
  int32_t count[2][EG_YEARS] = {};
  int64_t len[2] = {0, 0};
  int64_t size = 0;      // of its neighbourhood
  void finish(const eg_explore_opts& o) {
    for (int w = 0; w < 2; ++w) { len[w] = 0; for (int y = 0; y < EG_YEARS; ++y) len[w] += count[w][y]; }
    size = len[0] + len[1] + int64_t(o.n_replace) * len[0] + (len[0] < int64_t(snap::kBestCap) ? int64_t(EG_YEARS) * o.n_append : 0) +
           count_moves(count[0], o.max_shift);
  }
};
Base start_base(const eg_plan_set* starts, int32_t p, const eg_explore_opts& o) {
  Base b;
  b.number = p;
  for (int y = 0; y < EG_YEARS; ++y) { b.count[0][y] = starts->best_count[size_t(p) * EG_YEARS + y]; b.count[1][y] = starts->best_deficit_count[size_t(p) * EG_YEARS + y]; }
  b.finish(o);
  return b;
}
// one member's neighbourhood, in the header's order: the edits of a refinement round without its variant 0, then the moves
struct Hood {
  int64_t owner = -1;      // the position in the frontier of the member it was enumerated for
  std::vector<eg_plan_edit> edits;      // (edits[0] is the "none" the neighbourhood leaves out)
  std::vector<eg_plan_move> moves;
  void load(int64_t i, const Base& b, const eg_explore_opts& o) {
    if (owner == i) return;
    enumerate_edits(b.count[0], b.count[1], o.replace_with, o.n_replace, o.append_with, o.n_append, b.len[0] < int64_t(snap::kBestCap), edits);
    enumerate_moves(b.count[0], o.max_shift, moves);
    owner = i;
  }
  int64_t n_edits() const { return int64_t(edits.size()) - 1; }
};
// what an edit does to the length of list w
int delta(const eg_plan_edit& e, int w) { return e.list == w ? (e.kind == EG_EDIT_INSERT ? 1 : e.kind == EG_EDIT_DELETE ? -1 : 0) : 0; }
}  // namespace

extern "C" int32_t eg_explore_validate(const eg_plan_set* starts, const eg_explore_opts* xo) {
  auto fail = [](const std::string& m) { set_error("eg_explore_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(starts));
  EG_TRY(validate_front_opts(fail, starts, xo));
  EG_TRY(validate_action_lists(fail, xo->n_replace, xo->replace_with, xo->n_append, xo->append_with));
  if (xo->max_shift < 0 || xo->max_shift > EG_YEARS - 1)
    return fail("max_shift = " + std::to_string(xo->max_shift) + " (0.." + std::to_string(EG_YEARS - 1) + " years; 0: no moves)");
  EG_TRY(check_launch_variants(fail, xo->launch_variants));
  if (xo->max_variants < 0) return fail("max_variants = " + std::to_string(xo->max_variants) + " (0: no budget)");
  return EG_OK;
}

extern "C" int32_t eg_explore_neighbourhood(const eg_plan_set* starts, const eg_explore_opts* xo, int64_t* sizes) {
  EG_TRY(eg_explore_validate(starts, xo));
  if (!sizes) { set_error("eg_explore_neighbourhood: NULL sizes"); return EG_ERR_BAD_ARG; }
  for (int32_t p = 0; p < starts->n_plans; ++p) sizes[p] = start_base(starts, p, *xo).size;
  return EG_OK;
}

extern "C" int32_t eg_explore_plans(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* starts, const eg_explore_opts* xo, uint64_t seed,
                                    uint64_t episode_index, eg_plan_set** population, eg_explore_generation* generations, eg_explore_member* members,
                                    int64_t* final_numbers, int32_t* n_generations, int32_t* stop_reason, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !population || !generations || !members || !final_numbers || !n_generations || !stop_reason) {
    set_error(std::string(kFn) + ": bad argument"); return EG_ERR_BAD_ARG;
  }
  EG_TRY(plan_entry(c, s, o, kFn, [&] { return eg_explore_validate(starts, xo); }));
  const int64_t L = xo->launch_variants == 0 ? int64_t(EG_CROSS_MAX_VARIANTS) : int64_t(xo->launch_variants);
  const int32_t n = starts->n_plans;
  // the private archive (eg_breed_plans' buffer), started empty and kept through the call; generation 0: the start plans' blocks go up
  // into frontier array 0; no block goes up after this
  EG_TRY(archive_begin(c, xo->cap, xo->objectives, xo->mode));
  EG_TRY(archive_upload(c, starts, 0));
  DevSnapshot S{};
  EG_TRY(stage_eval_snapshot(c, s, o, &S));
  std::vector<Base> F, next;      // the frontier: member i's block is block base_at + i of frontier array `cur`
  for (int32_t p = 0; p < n; ++p) F.push_back(start_base(starts, p, *xo));
  const std::vector<Base> start = F;
  int cur = 0;
  uint32_t base_at = 0;
  int64_t number = 0;      // of the next variant
  Hood hood;
  std::vector<uint8_t> in, rb;
  Routing R;
  std::vector<int64_t> first_of;      // the number of every member's first neighbour
  *n_generations = 0; *stop_reason = EG_EXPLORE_MAX_GENERATIONS; *population = nullptr;
  int32_t n_held = 0;
  for (int32_t g = 0; g < xo->max_generations; ++g) {
    const std::string at = std::string(kFn) + ": generation " + std::to_string(g) + ": ";
    eg_explore_generation& G = generations[g];
    G = eg_explore_generation{};
    G.n_frontier = int32_t(F.size());
    const int64_t nones = g == 0 ? n : 0, gen_first = number, m_first = gen_first + nones;
    first_of.assign(F.size(), 0);
    int64_t V = nones;
    for (size_t i = 0; i < F.size(); ++i) { first_of[i] = gen_first + V; V += F[i].size; }
    G.n_variants = V;
    const uint32_t n_bases = base_at + uint32_t(F.size());
    if (V > 0) {
      const uint32_t n_cap = uint32_t(std::min<int64_t>(V, L));
      EG_TRY(ensure_outputs(c, n_cap));
      EG_HIP(c->d_plans.reserve(size_t(n_cap) * snap::kPlanStride));
      EG_HIP(c->d_plan_index.reserve(n_cap));
      EG_HIP(c->d_refine_in.reserve(size_t(n_cap) * 12));
      S.plan_pool = c->d_plans;      // (the pool may have been a smaller one, or none, when the snapshot was staged)
    }
    hood.owner = -1;
    int64_t none_at = 0;      // generation 0: the start plans still to ride as "none" edits
    size_t ci = 0;            // the member whose neighbourhood is being cut, and how much of it has gone
    int64_t ck = 0;
    for (int64_t done = 0; done < V;) {
      const uint32_t m = uint32_t(std::min<int64_t>(V - done, L));
      // what goes up in one copy: the packed edits and moves (8 bytes a variant), then every variant's slot; and the routing — the
      // short variants of the chunk first, then the long ones (launch_plans)
      in.assign(size_t(m) * 12, 0);
      uint32_t* packed = reinterpret_cast<uint32_t*>(in.data());
      uint32_t* slot = reinterpret_cast<uint32_t*>(in.data() + size_t(m) * 8);
      R.clear();
      bool any_moves = false;
      uint32_t j = 0;
      for (; nones > none_at && j < m; ++j, ++none_at) {      // (packed zeros: "none")
        slot[j] = uint32_t(none_at);
        R.add(j, F[size_t(none_at)].len[0]);
      }
      while (j < m) {
        while (ci < F.size() && ck == F[ci].size) { ++ci; ck = 0; }      // (V counts what is left: there is a member with variants to give)
        if (ci >= F.size()) { set_error(at + "the frontier ran out before its variant count"); return EG_ERR_INTERNAL; }
        const Base& b = F[ci];
        hood.load(int64_t(ci), b, *xo);
        if (hood.n_edits() + int64_t(hood.moves.size()) != b.size) { set_error(at + "the enumeration and its count disagree"); return EG_ERR_INTERNAL; }
        const uint32_t take = uint32_t(std::min<int64_t>(int64_t(m - j), b.size - ck));
        // (the part [ck, ck + take) of the neighbourhood: what is left of its edits, then moves)
        const int64_t e0 = std::min(ck, hood.n_edits()), n_e = std::min<int64_t>(hood.n_edits() - e0, take);
        if (pack_neighbourhood(base_at + uint32_t(ci), b.len[0], hood.edits.data() + 1 + e0, uint32_t(n_e), hood.moves.data() + (ck - e0), take - uint32_t(n_e), j, packed, slot, R))
          any_moves = true;
        j += take; ck += take;
      }
      EG_TRY(launch_variants(c, S, archive_array(c, cur), n_bases, in, size_t(m) * 8, m, R, any_moves, seed, episode_index));
      EG_TRY(archive_fold(c, m, uint64_t(number)));
      done += m; number += m;
    }
    // (generation 0: the start plans the archive holds entered in it too — their rows are row 0 of `members` — so everything held is new)
    EG_LAUNCH("k_explore_turnover", launch_explore_turnover(c->d_breed, 1 - cur, g == 0 ? 0 : m_first, nullptr));
    EG_TRY(archive_read_generation(c, rb));
    ExploreHeader h{};
    std::memcpy(&h, rb.data(), sizeof(h));
    if (h.n_held < 0 || h.n_held > xo->cap || h.n_new < 0 || h.n_new > h.n_held || h.n_valid < 0 || h.n_valid > V || h.n_dropped < 0 ||
        (g == 0 && ((h.n_held == 0) != (h.n_valid == 0) || h.n_new != h.n_held)) || (g > 0 && h.n_held == 0)) {
      set_error(at + "the device's readback header is corrupt"); return EG_ERR_INTERNAL;
    }
    G.n_held = n_held = h.n_held; G.n_valid = h.n_valid; G.n_dropped = h.n_dropped;
    *n_generations = g + 1;
    if (h.n_held == 0) {      // no valid variant: the start plans stand in frontier array 0
      *stop_reason = EG_EXPLORE_EMPTY;
      return decode_device_blocks(archive_array(c, 0), n, nullptr, kFn, population);
    }
    next.clear();
    uint32_t n_starts_held = 0;
    long long before = -1;
    hood.owner = -1;
    for (int32_t r = 0; r < h.n_new; ++r) {
      ParetoEntry e{};
      Base b;
      int32_t tab[2][28];
      bool ok = archive_row(rb, r, xo->cap, &e, tab) && e.index > before && e.index >= (g == 0 ? 0 : m_first) && e.index < gen_first + V;
      eg_explore_member M{};
      if (ok) {
        for (int w = 0; w < 2; ++w) for (int y = 0; y < EG_YEARS; ++y) b.count[w][y] = tab[w][y + 1] - tab[w][y];
        b.number = e.index; b.finish(*xo);
        M.number = e.index; M.score = e.score;
        std::memcpy(M.metrics, e.metrics, sizeof(M.metrics));
        if (e.index < m_first) {      // a start plan, riding as a "none" edit
          const Base& from = start[size_t(e.index)];
          M.parent = -1;
          ok = b.len[0] == from.len[0] && b.len[1] == from.len[1];
        } else {
          // the member whose neighbourhood holds the number, and the variant there; the block against the host's count
          const size_t i = size_t(std::upper_bound(first_of.begin(), first_of.end(), int64_t(e.index)) - first_of.begin()) - 1;
          const int64_t k = e.index - first_of[i];
          const Base& from = F[i];
          ok = k >= 0 && k < from.size;
          if (ok) {
            hood.load(int64_t(i), from, *xo);
            M.parent = from.number;
            if (k < hood.n_edits()) {
              M.edit = hood.edits[size_t(1 + k)];
              ok = b.len[0] == from.len[0] + delta(M.edit, 0) && b.len[1] == from.len[1] + delta(M.edit, 1);
            } else {
              M.is_move = 1; M.move = hood.moves[size_t(k - hood.n_edits())];
              ok = b.len[0] == from.len[0] && b.len[1] == from.len[1];
            }
          }
        }
      }
      if (!ok) { set_error(at + "the device's readback row " + std::to_string(r) + " does not describe a variant of the generation"); return EG_ERR_INTERNAL; }
      before = e.index;
      if (e.index < m_first) members[size_t(n_starts_held++)] = M;
      else { members[size_t(g + 1) * size_t(xo->cap) + next.size()] = M; next.push_back(b); }
    }
    G.n_new = int32_t(next.size());
    cur = 1 - cur; base_at = n_starts_held;
    F.swap(next);
    if (F.empty()) { *stop_reason = EG_EXPLORE_EXPLORED; break; }
    int64_t want = 0;
    for (const Base& b : F) want += b.size;
    if (xo->max_variants > 0 && number + want > xo->max_variants) { *stop_reason = EG_EXPLORE_BUDGET; break; }
  }
  // the archive as it stands: its entries in ascending number, each naming its record slot, beside which its block is kept
  std::vector<ParetoEntry> held((size_t(n_held)));
  EG_HIP(hipMemcpy(held.data(), c->d_breed + offsetof(ParetoState, e), held.size() * sizeof(ParetoEntry), hipMemcpyDeviceToHost));
  std::vector<int32_t> slots((size_t(n_held)));
  for (int32_t r = 0; r < n_held; ++r) {
    const ParetoEntry& e = held[size_t(r)];
    if (e.index < (r ? held[size_t(r) - 1].index + 1 : 0) || e.index >= number || e.slot < 0 || e.slot >= xo->cap) {
      set_error(std::string(kFn) + ": entry " + std::to_string(r) + " of the archive on the device is corrupt"); return EG_ERR_INTERNAL;
    }
    final_numbers[r] = e.index; slots[size_t(r)] = e.slot;
    EG_TRY(archive_fetch_record(c, e.slot, out, size_t(r)));
  }
  return decode_device_blocks(c->d_breed + breed_at::blocks, n_held, slots.data(), kFn, population);
}
