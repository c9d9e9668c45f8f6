"""Host-side mirror of the reference interface for the rollout hot path, on top of the C ABI.

Names follow the reference: `ActionWeights` (ai/learning/weights/mod.rs:50-107), `run_iteration`
(core/iteration.rs:10-20), `SimulationMetrics` (ai/metrics/simulation_metrics.rs:5-11), `find_suitable_location`
(gpu/metal_location_search.rs:96-103).  All compute happens in libeirgrid_hip.so on the GPU; this file only
marshals numpy buffers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields

import numpy as np

from . import _native as N
from .constraints import BuildConstraint, Constraint, build_constraint_array, constraint_array, constraint_list, split_constraints
from .world import World

BASE_YEAR, END_YEAR = 2025, 2050

YEARLY_COLUMNS = [
    "year", "total_population", "total_power_usage", "total_power_generation", "power_balance",
    "average_public_opinion", "yearly_capital_cost", "total_capital_cost", "inflation_factor", "total_co2_emissions",
    "total_carbon_offset", "net_co2_emissions", "yearly_carbon_credit_revenue", "total_carbon_credit_revenue",
    "yearly_energy_sales_revenue", "total_energy_sales_revenue", "active_generators", "yearly_upgrade_costs",
    "yearly_closure_costs", "yearly_total_cost", "total_cost",
]


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _world_struct(world: World):
    keep = [np.ascontiguousarray(world.settlement_x, dtype=np.float64), np.ascontiguousarray(world.settlement_y, dtype=np.float64),
            np.ascontiguousarray(world.settlement_pop, dtype=np.uint32),
            np.ascontiguousarray(world.existing_x, dtype=np.float64), np.ascontiguousarray(world.existing_y, dtype=np.float64),
            np.ascontiguousarray(world.existing_type, dtype=np.int32), np.ascontiguousarray(world.existing_capacity, dtype=np.float64),
            np.ascontiguousarray(world.coast_x, dtype=np.float64), np.ascontiguousarray(world.coast_y, dtype=np.float64)]
    w = N.EgWorld(len(keep[0]), _p(keep[0], C.c_double), _p(keep[1], C.c_double), _p(keep[2], C.c_uint32),
                  len(keep[3]), _p(keep[3], C.c_double), _p(keep[4], C.c_double), _p(keep[5], C.c_int32), _p(keep[6], C.c_double),
                  len(keep[7]), _p(keep[7], C.c_double), _p(keep[8], C.c_double), int(world.existing_operational_at_start))
    return w, keep


class HostTables:
    """The policy-independent tables the library builds on the host for a world (no device needed)."""

    def __init__(self, world: World):
        w, self._keep = _world_struct(world)
        self.h = N.lib().eg_host_tables_create(C.byref(w))
        if not self.h:
            raise N.EirgridError(N.lib().eg_last_error().decode())

    def __del__(self):
        if getattr(self, "h", None):
            N.lib().eg_host_tables_free(self.h)
            self.h = None

    def f64(self, name: str) -> np.ndarray:
        ptr, n = C.POINTER(C.c_double)(), C.c_int64()
        N.check(N.lib().eg_host_tables_f64(self.h, name.encode(), C.byref(ptr), C.byref(n)), "eg_host_tables_f64")
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()

    def i32(self, name: str) -> np.ndarray:
        ptr, n = C.POINTER(C.c_int32)(), C.c_int64()
        N.check(N.lib().eg_host_tables_i32(self.h, name.encode(), C.byref(ptr), C.byref(n)), "eg_host_tables_i32")
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()


class ActionWeights:
    """ActionWeights held by the library (eg_policy): tables, best strategy, counters."""
    SC = dict(learning_rate=0, exploration_rate=1, iterations_without_improvement=2, iteration_count=3, has_best=4,
              best_net_emissions=5, best_opinion=6, best_cost=7, best_reliability=8, has_best_actions=9,
              has_best_deficit_actions=10, has_count_weights=11, improvement_history_len=12, failed_episodes=13)

    def __init__(self, handle=None):
        self.h = handle if handle is not None else N.lib().eg_policy_new()

    def save_to_file(self, path: str) -> None:
        """ai/learning/weights/serialization.rs:29-139 — pretty JSON in the reference's SerializableWeights schema."""
        N.check(N.lib().eg_policy_save_json(self.h, str(path).encode()), "eg_policy_save_json")

    @staticmethod
    def load_from_file(path: str) -> "ActionWeights":
        """ai/learning/weights/serialization.rs:140-493."""
        h = N.lib().eg_policy_load_json(str(path).encode())
        if not h:
            raise N.EirgridError(N.lib().eg_last_error().decode())
        return ActionWeights(h)

    def __del__(self):
        if getattr(self, "h", None):
            try:
                N.lib().eg_policy_free(self.h)
            except TypeError:      # interpreter shutdown: module globals are already gone
                pass
            self.h = None

    def tables(self):
        w = np.zeros((N.YEARS, N.N_ACTIONS)); dw = np.zeros((N.YEARS, N.N_DEFICIT)); cw = np.zeros((N.YEARS, N.N_COUNTS))
        N.check(N.lib().eg_policy_get_tables(self.h, _p(w, C.c_double), _p(dw, C.c_double), _p(cw, C.c_double)))
        return w, dw, cw

    def set_tables(self, w=None, dw=None, cw=None):
        args, keep = [], []
        for a in (w, dw, cw):
            if a is None:
                args.append(None)
            else:
                a = np.ascontiguousarray(a, dtype=np.float64); keep.append(a); args.append(_p(a, C.c_double))
        N.check(N.lib().eg_policy_set_tables(self.h, *args))

    def get(self, name: str) -> float:
        return N.lib().eg_policy_get_scalar(self.h, self.SC[name])

    def set(self, name: str, v) -> None:
        N.check(N.lib().eg_policy_set_scalar(self.h, self.SC[name], float(v)))

    def get_list(self, which: int, yi: int):
        buf = (C.c_uint8 * 4096)()
        n = N.lib().eg_policy_get_list(self.h, which, yi, buf, 4096)
        return list(buf[:n])

    def lists(self, which: int):
        return [self.get_list(which, y) for y in range(N.YEARS)]

    def snapshot(self) -> N.EgPolicySnapshot:
        s = N.EgPolicySnapshot()
        N.check(N.lib().eg_policy_snapshot_view(self.h, C.byref(s)))
        return s

    def apply_episode(self, metrics, n_run, run_log, n_def, def_log, noise_seed: int = 0):
        """core/multi_simulation.rs:494-508 for one finished episode."""
        m = np.ascontiguousarray(metrics, dtype=np.float64)
        nr = np.ascontiguousarray(n_run, dtype=np.int32); nd = np.ascontiguousarray(n_def, dtype=np.int32)
        rl = np.ascontiguousarray(run_log, dtype=np.uint8); dl = np.ascontiguousarray(def_log, dtype=np.uint8)
        N.check(N.lib().eg_policy_apply_episode(self.h, _p(m, C.c_double), _p(nr, C.c_int32), _p(rl, C.c_uint8),
                                                _p(nd, C.c_int32), _p(dl, C.c_uint8), C.c_uint64(noise_seed)))


def apply_reduced(weights: "ActionWeights", stats, candidate, noise_seed: int = 0) -> bool:
    """Batch form of core/multi_simulation.rs:494-508 (SURVEY.md §8(e) reduced mode).  `stats` is the all-reduced host copy
    of the eg_update_stats buffer (int64[STATS_LEN]); `candidate` = (metrics, n_run, run_log, n_def, def_log) of the batch's
    best episode or None.  Returns True when the candidate became the best strategy."""
    st = np.ascontiguousarray(stats, dtype=np.int64)
    assert st.shape == (N.STATS_LEN,)
    if candidate is None:
        rc = N.lib().eg_policy_apply_reduced(weights.h, _p(st, C.c_int64), None, None, None, None, None, C.c_uint64(noise_seed))
    else:
        m = np.ascontiguousarray(candidate[0], dtype=np.float64)
        nr = np.ascontiguousarray(candidate[1], dtype=np.int32); rl = np.ascontiguousarray(candidate[2], dtype=np.uint8)
        nd = np.ascontiguousarray(candidate[3], dtype=np.int32); dl = np.ascontiguousarray(candidate[4], dtype=np.uint8)
        rc = N.lib().eg_policy_apply_reduced(weights.h, _p(st, C.c_int64), _p(m, C.c_double), _p(nr, C.c_int32), _p(rl, C.c_uint8),
                                             _p(nd, C.c_int32), _p(dl, C.c_uint8), C.c_uint64(noise_seed))
    if rc < 0:
        N.check(rc, "eg_policy_apply_reduced")
    return rc == 1


def apply_packet(weights: "ActionWeights", stats, candidates, noise_seed: int = 0) -> bool:
    """eg_policy_apply_packet: `stats` int64[STATS_LEN] (all-reduced), `candidates` uint8[W, CANDIDATE_BYTES] candidate
    records, one per rank.  The winner (highest score, ties to the lowest global index) competes for the best slot."""
    st = np.ascontiguousarray(stats, dtype=np.int64)
    cd = np.ascontiguousarray(candidates, dtype=np.uint8).reshape(-1, N.CANDIDATE_BYTES)
    assert st.shape == (N.STATS_LEN,)
    rc = N.lib().eg_policy_apply_packet(weights.h, st.ctypes.data, cd.ctypes.data, cd.shape[0], C.c_uint64(noise_seed))
    if rc < 0:
        N.check(rc, "eg_policy_apply_packet")
    return rc == 1


def evaluate_action_impact(current_metrics, new_metrics, cost_only: bool = False) -> float:
    """ai/metrics/scoring.rs:46-85 on SimulationMetrics quadruples (metrics_to_action_result, multi_simulation.rs:55-62)."""
    a = np.ascontiguousarray(current_metrics, dtype=np.float64); b = np.ascontiguousarray(new_metrics, dtype=np.float64)
    return N.lib().eg_evaluate_action_impact(_p(a, C.c_double), _p(b, C.c_double), int(cost_only))


def score_metrics(metrics, cost_only: bool = False) -> float:
    m = np.ascontiguousarray(metrics, dtype=np.float64)
    return N.lib().eg_score_metrics(_p(m, C.c_double), int(cost_only))


def rank_score(metrics, cost_only: bool = False) -> float:
    """The top-K archive's rank score (eg_rank_score): score_metrics with the library's own logarithm, the bits the device uses."""
    m = np.ascontiguousarray(metrics, dtype=np.float64)
    return N.lib().eg_rank_score(_p(m, C.c_double), 2 if cost_only else 1)


@dataclass
class Ensemble:
    """The eg_ensemble_row of every variant of a batch that ran under plan streams (Engine.fetch_ensemble), as arrays over the variants."""
    nominal: np.ndarray        # [n, 4] stream 0's metrics
    committed: np.ndarray      # [n, 4] what the records hold
    score_min: np.ndarray      # [n] the smallest / largest stream score that is not NaN (NaN: every score is)
    score_max: np.ndarray
    score_sum: np.ndarray      # [n] the stream scores added in ascending stream order
    n_ok: np.ndarray           # [n] int32: streams that ended EG_EP_OK / EG_EP_INFEASIBLE / any other way
    n_infeasible: np.ndarray
    n_failed: np.ndarray
    worst_stream: np.ndarray   # [n] int32: the first stream of the order (a NaN score, then the smallest score, then the lowest stream)
    status: np.ndarray         # [n] int32 the committed status


def ensemble_reduce(metrics, status, tail: int, cost_only: bool = False) -> dict:
    """The reduction of one variant's R streams (include/eirgrid_hip.h, plan streams), restated with sequential Python adds: metrics
    [R, 4], status [R].  Returns the eg_ensemble_row as a dict — nominal and committed as float64 arrays of 4, the scores, the counters,
    worst_stream and status — bit for bit what k_ensemble_commit writes."""
    m = np.ascontiguousarray(metrics, dtype=np.float64)
    st = [int(t) for t in status]
    R = len(st)
    if m.shape != (R, 4) or not 1 <= R <= N.STREAMS_MAX or not 1 <= int(tail) <= R:
        raise ValueError(f"ensemble_reduce: metrics {m.shape}, {R} statuses, tail {tail}")
    s = [np.float64(rank_score(m[r], cost_only)) for r in range(R)]

    def before(q, r):      # stream q comes before stream r: a NaN score first, then the smaller score, then the lower stream
        if s[q] != s[q]:
            return s[r] == s[r] or q < r
        return s[r] == s[r] and (s[q] < s[r] or (s[q] == s[r] and q < r))

    rank = [sum(1 for q in range(R) if before(q, r)) for r in range(R)]
    selected = [r for r in range(R) if rank[r] < int(tail)]
    committed = np.zeros(4, np.float64)
    with np.errstate(all="ignore"):
        for i in range(4):
            c = m[selected[0], i]
            for r in selected[1:]:
                c = c + m[r, i]
            committed[i] = c / np.float64(tail)
        score_sum = s[0]
        for r in range(1, R):
            score_sum = score_sum + s[r]
    score_min = score_max = None
    for r in range(R):
        if s[r] == s[r]:
            score_min = s[r] if score_min is None or s[r] < score_min else score_min
            score_max = s[r] if score_max is None or s[r] > score_max else score_max
    bad = [r for r in range(R) if st[r] != N.EG_EP_OK]
    n_ok, n_inf = R - len(bad), sum(1 for t in st if t == N.EG_EP_INFEASIBLE)
    return {"nominal": m[0].copy(), "committed": committed, "score_min": np.float64(np.nan) if score_min is None else score_min,
            "score_max": np.float64(np.nan) if score_max is None else score_max, "score_sum": np.float64(score_sum), "n_ok": n_ok, "n_infeasible": n_inf,
            "n_failed": R - n_ok - n_inf, "worst_stream": rank.index(0), "status": st[bad[0]] if bad else N.EG_EP_OK}


class Plan:
    """A strategy to score (eg_evaluate_plans): per year the best_actions list and the best_deficit_actions list, canonical action
    indices 0..60 — what update_best_strategy installs and a replay episode reads."""

    def __init__(self, best_actions, best_deficit_actions, name: str = ""):
        self.best_actions = [list(map(int, best_actions[y])) for y in range(N.YEARS)]
        self.best_deficit_actions = [list(map(int, best_deficit_actions[y])) for y in range(N.YEARS)]
        self.name = name
        assert len(best_actions) == N.YEARS and len(best_deficit_actions) == N.YEARS

    def __len__(self) -> int:
        """Entries of the best_actions list (what routes a plan to the short or the long replay path)."""
        return sum(len(l) for l in self.best_actions)

    def __eq__(self, other) -> bool:
        return isinstance(other, Plan) and (self.best_actions, self.best_deficit_actions) == (other.best_actions, other.best_deficit_actions)

    def __repr__(self) -> str:
        return f"Plan({self.name!r}, {len(self)} actions, {sum(len(l) for l in self.best_deficit_actions)} deficit actions)"

    @staticmethod
    def _from_set(s) -> "list[Plan]":
        out, pos, dpos = [], 0, 0
        for j in range(s.n_plans):
            run, dfc = [], []
            for y in range(N.YEARS):
                k, dk = s.best_count[j * N.YEARS + y], s.best_deficit_count[j * N.YEARS + y]
                run.append(list(s.best_actions[pos:pos + k])); dfc.append(list(s.best_deficit_actions[dpos:dpos + dk]))
                pos += k; dpos += dk
            out.append(Plan(run, dfc, s.names[j].decode() if s.names else ""))
        return out

    @staticmethod
    def _take_set(ps) -> "list[Plan]":
        """the plans of a set the library returned (eg_plan_set *), which is freed"""
        try:
            return Plan._from_set(ps.contents)
        finally:
            N.lib().eg_plans_free(ps)

    @staticmethod
    def load(path: str) -> "list[Plan]":
        """Plans of a file in the checkpoint schema: one checkpoint (one plan) or JSON Lines with optional names (eg_plans_load)."""
        L = N.lib()
        ps = L.eg_plans_load(str(path).encode())
        if not ps:
            raise N.EirgridError(L.eg_last_error().decode())
        return Plan._take_set(ps)

    @staticmethod
    def save(path: str, plans) -> None:
        """The plans as JSON Lines in the checkpoint schema (eg_plans_save): what Plan.load and --evaluate read."""
        ps = plans if isinstance(plans, PlanSet) else PlanSet(plans)
        N.check(N.lib().eg_plans_save(C.byref(ps.s), str(path).encode()), "eg_plans_save")

    @staticmethod
    def from_policy(weights: "ActionWeights", name: str = "") -> "Plan":
        """The policy's current best lists (empty when it has none)."""
        return Plan(weights.lists(0), weights.lists(1), name)

    @staticmethod
    def from_result(res: "BatchResult", e: int, name: str = "") -> "Plan":
        """The lists update_best_strategy would install from episode e: its current_run_actions / current_deficit_actions by year
        (ai/learning/strategy.rs)."""
        return Plan(res.lists(e, "run"), res.lists(e, "def"), name)


class PlanSet:
    """Plans as one eg_plan_set (the arrays stay alive as long as this object)."""

    def __init__(self, plans):
        plans = list(plans)
        self.count = np.array([[len(l) for l in p.best_actions] for p in plans], np.int32).reshape(len(plans), N.YEARS)
        self.dcount = np.array([[len(l) for l in p.best_deficit_actions] for p in plans], np.int32).reshape(len(plans), N.YEARS)
        self.act = np.array([a for p in plans for l in p.best_actions for a in l] or [0], np.uint8)
        self.dact = np.array([a for p in plans for l in p.best_deficit_actions for a in l] or [0], np.uint8)
        self.names = (C.c_char_p * max(len(plans), 1))(*[p.name.encode() for p in plans])
        self.s = N.EgPlanSet(len(plans), _p(self.count, C.c_int32), _p(self.act, C.c_uint8), _p(self.dcount, C.c_int32),
                             _p(self.dact, C.c_uint8), int(self.count.sum()), int(self.dcount.sum()), self.names)


@dataclass(frozen=True)
class PlanEdit:
    """One edit of a plan (eg_plan_edit): kind "none" (the plan itself), "delete", "replace" or "insert" (in front of `pos`; pos = len
    appends); list 0 = best_actions, 1 = best_deficit_actions; year: the year index 0..25; pos: a position in that year's list; action:
    the canonical index replace / insert put there."""
    kind: str = "none"
    list: int = 0
    year: int = 0
    pos: int = 0
    action: int = 0

    KINDS = ("none", "delete", "replace", "insert")

    def struct(self) -> N.EgPlanEdit:
        return N.EgPlanEdit(self.KINDS.index(self.kind), self.list, self.year, self.pos, self.action)

    def apply(self, plan: "Plan") -> "Plan":
        """The edited plan (a copy), as the device builds it."""
        lists = ([list(l) for l in plan.best_actions], [list(l) for l in plan.best_deficit_actions])
        l = lists[self.list][self.year]
        if self.kind == "delete":
            del l[self.pos]
        elif self.kind == "replace":
            l[self.pos] = self.action
        elif self.kind == "insert":
            l.insert(self.pos, self.action)
        return Plan(lists[0], lists[1], plan.name)


@dataclass(frozen=True)
class PlanMove:
    """One move of a plan (eg_plan_move): entry `pos` of year `year` of a list (0 = best_actions, 1 = best_deficit_actions) is taken out
    and put back in front of entry `to_pos` of year `to_year`'s list as that list stands after the removal (to_pos = its length: behind
    the last entry).  to_year == year reorders within the year; with to_pos == pos as well the move is the plan itself."""
    list: int = 0
    year: int = 0
    pos: int = 0
    to_year: int = 0
    to_pos: int = 0

    def struct(self) -> N.EgPlanMove:
        return N.EgPlanMove(self.list, self.to_year, self.year, self.pos, self.to_pos)

    def apply(self, plan: "Plan") -> "Plan":
        """The moved plan (a copy), as the device builds it."""
        lists = ([list(l) for l in plan.best_actions], [list(l) for l in plan.best_deficit_actions])
        a = lists[self.list][self.year].pop(self.pos)
        lists[self.list][self.to_year].insert(self.to_pos, a)
        return Plan(lists[0], lists[1], plan.name)


def _move_array(moves):
    moves = list(moves)
    arr = (N.EgPlanMove * max(len(moves), 1))()
    for j, m in enumerate(moves):
        arr[j] = m.struct() if isinstance(m, PlanMove) else m
    return arr, len(moves)


def refine_moves(base: "Plan", max_shift: int) -> "list[PlanMove]":
    """The move variants of one round of Engine.refine_plans(..., max_shift): every best_actions entry in (year, position) order, and
    per entry each shift d = -1, +1, -2, +2, ..., -max_shift, +max_shift that stays inside the 26 years: the entry moved behind the
    last entry of year year + d."""
    return [PlanMove(0, y, i, y + d, len(base.best_actions[y + d])) for y, l in enumerate(base.best_actions) for i in range(len(l))
            for s in range(1, int(max_shift) + 1) for d in (-s, s) if 0 <= y + d < N.YEARS]


@dataclass(frozen=True)
class PlanCross:
    """One cross of two plans of a parent set (eg_plan_cross): parent `a` with BOTH lists of the years from_year <= y < to_year replaced
    by parent `b`'s lists of those years (0 <= from_year <= to_year <= 26).  from_year == to_year or a == b is parent a itself;
    to_year == 26 is the one-point crossover (head of a, tail of b); to_year == from_year + 1 transplants one year."""
    a: int = 0
    b: int = 0
    from_year: int = 0
    to_year: int = 0

    def struct(self) -> N.EgPlanCross:
        return N.EgPlanCross(self.a, self.b, self.from_year, self.to_year)

    def apply(self, parents) -> "Plan":
        """The child (a new plan, named after parent a), as the device builds it."""
        pa, pb = parents[self.a], parents[self.b]
        take = lambda la, lb: [list(lb[y] if self.from_year <= y < self.to_year else la[y]) for y in range(N.YEARS)]
        return Plan(take(pa.best_actions, pb.best_actions), take(pa.best_deficit_actions, pb.best_deficit_actions), pa.name)


def _cross_array(crosses):
    crosses = list(crosses)
    arr = (N.EgPlanCross * max(len(crosses), 1))()
    for j, x in enumerate(crosses):
        arr[j] = x.struct() if isinstance(x, PlanCross) else x
    return arr, len(crosses)


@dataclass(frozen=True)
class ActionMap:
    """An action map (eg_action_map): `to[e]` is what entry e of a plan list becomes, an action 0..60 or ActionMap.DROP (0xFF): e is taken
    out.  An action is 3 * type + cost tier for the generator types (0..44, world.GENERATOR_TYPE_NAMES; tier 0 is the 100 % one) and
    the carbon offsets (45..56); 57..60 have no tiers."""
    to: tuple

    DROP = N.REWRITE_DROP
    N_TIERED = 57      # the actions below it come in three cost tiers

    def __post_init__(self):
        to = tuple(int(t) for t in self.to)
        if len(to) != N.N_ACTIONS or any(not (0 <= t < N.N_ACTIONS or t == self.DROP) for t in to):
            raise ValueError(f"ActionMap: {N.N_ACTIONS} entries, each an action 0..{N.N_ACTIONS - 1} or {self.DROP} (drop)")
        object.__setattr__(self, "to", to)

    def struct(self) -> N.EgActionMap:
        return N.EgActionMap((C.c_uint8 * N.N_ACTIONS)(*self.to))

    @staticmethod
    def identity() -> "ActionMap":
        return ActionMap(tuple(range(N.N_ACTIONS)))

    @staticmethod
    def substitute(pairs) -> "ActionMap":
        """a becomes b for every a: b of `pairs`; every other action stays"""
        to = list(range(N.N_ACTIONS))
        for a, b in dict(pairs).items():
            to[int(a)] = int(b)
        return ActionMap(tuple(to))

    @staticmethod
    def drop(actions) -> "ActionMap":
        return ActionMap.substitute({int(a): ActionMap.DROP for a in actions})

    @staticmethod
    def drop_technology(type_index: int) -> "ActionMap":
        """the three cost tiers of generator type `type_index` dropped"""
        return ActionMap.drop(range(3 * int(type_index), 3 * int(type_index) + 3))

    @staticmethod
    def replace_technology(t: int, u: int) -> "ActionMap":
        """generator type t built as type u at the same cost tier"""
        return ActionMap.substitute({3 * int(t) + k: 3 * int(u) + k for k in range(3)})

    @staticmethod
    def cost_tier(k: int) -> "ActionMap":
        """every generator and offset action at cost tier k (0, 1 or 2)"""
        if int(k) not in (0, 1, 2):
            raise ValueError(f"ActionMap.cost_tier: tier {k} (0, 1 or 2)")
        return ActionMap(tuple(a - a % 3 + int(k) if a < ActionMap.N_TIERED else a for a in range(N.N_ACTIONS)))

    @staticmethod
    def drop_all() -> "ActionMap":
        return ActionMap((ActionMap.DROP,) * N.N_ACTIONS)


@dataclass(frozen=True)
class PlanRewrite:
    """One rewrite of a plan of a set (eg_plan_rewrite): plan `plan` with map `map` of a list of maps applied to every entry of the years
    from_year <= y < to_year of the selected lists (`lists`: bit 0 best_actions, bit 1 best_deficit_actions) — an entry e becomes to[e]
    or is taken out, the order kept.  lists == 0 or from_year == to_year is the plan itself.  A best_deficit_actions list that runs short
    is refilled by seeded draws from the fallback distribution (gas peakers among them): substitute there, do not drop."""
    plan: int = 0
    map: int = 0
    from_year: int = 0
    to_year: int = N.YEARS
    lists: int = 1

    def struct(self) -> N.EgPlanRewrite:
        return N.EgPlanRewrite(self.plan, self.map, self.from_year, self.to_year, self.lists, 0)

    def apply(self, plans, maps) -> "Plan":
        """The child (a new plan, named after the plan), as the device builds it."""
        p, to = plans[self.plan], maps[self.map].to
        def take(lists, bit):
            if not self.lists >> bit & 1:
                return [list(l) for l in lists]
            return [[to[e] for e in l if to[e] != ActionMap.DROP] if self.from_year <= y < self.to_year else list(l) for y, l in enumerate(lists)]
        return Plan(take(p.best_actions, 0), take(p.best_deficit_actions, 1), p.name)


def _map_array(maps):
    maps = list(maps)
    arr = (N.EgActionMap * max(len(maps), 1))()
    for j, m in enumerate(maps):
        arr[j] = m.struct() if isinstance(m, ActionMap) else m
    return arr, len(maps)


def _rewrite_array(rewrites):
    rewrites = list(rewrites)
    arr = (N.EgPlanRewrite * max(len(rewrites), 1))()
    for j, r in enumerate(rewrites):
        arr[j] = r.struct() if isinstance(r, PlanRewrite) else r
    return arr, len(rewrites)


@dataclass(frozen=True)
class TechnologyRow:
    """A row of Engine.technology_report: plan `plan` without generator type `type` (-1: the plan itself), the best_actions entries that
    took out, the variant's status, four metrics and rank score, and the score minus the plan's own."""
    plan: int
    type: int
    removed: int
    status: int
    metrics: tuple
    score: float
    delta: float


def technology_rewrites(plans, deficit: str = "substitute", substitute_with: int = 3 * 12):
    """The variants of Engine.technology_report: (parents, maps, rewrites, rows), rows[j] = (plan, type, entries removed) of rewrites[j]
    over `parents` and `maps`.  Per plan the plan itself (type -1), then per generator type t its best_actions uses, ascending, the
    plan without t: the three tiers of t dropped from best_actions.  With deficit == "substitute" every tier of t in
    best_deficit_actions becomes `substitute_with` as well; a variant applies ONE map, so where the deficit list does hold t the plan
    with that list substituted on the host rides in `parents` behind the plans, and the variant drops t from ITS best_actions."""
    if deficit not in ("substitute", "keep"):
        raise ValueError(f"technology_report: deficit = {deficit!r} (\"substitute\" or \"keep\")")
    if not 0 <= int(substitute_with) < N.N_ACTIONS:
        raise ValueError(f"technology_report: substitute_with = {substitute_with} (an action 0..{N.N_ACTIONS - 1})")
    parents, maps, slot, rewrites, rows = list(plans), [ActionMap.identity()], {}, [], []
    for p, plan in enumerate(plans):
        rewrites.append(PlanRewrite(p, 0, 0, 0, 0)); rows.append((p, -1, 0))
        used = [a for l in plan.best_actions for a in l]
        in_deficit = {a // 3 for l in plan.best_deficit_actions for a in l}
        for t in sorted({a // 3 for a in used if a < 3 * N.N_TYPES}):
            if t not in slot:
                slot[t] = len(maps); maps.append(ActionMap.drop_technology(t))
            src = p
            if deficit == "substitute" and t in in_deficit:
                sub = ActionMap.substitute({3 * t + k: int(substitute_with) for k in range(3)})
                src = len(parents); parents.append(PlanRewrite(0, 0, 0, N.YEARS, 2).apply([plan], [sub]))
            rewrites.append(PlanRewrite(src, slot[t], 0, N.YEARS, 1)); rows.append((p, t, sum(1 for a in used if a // 3 == t)))
    return parents, maps, rewrites, rows


def cross_pairs(n_plans: int, cuts=range(1, 26)) -> "list[PlanCross]":
    """The variants of Engine.cross_front over n_plans parents: every parent itself, PlanCross(p, p, 0, 0), in order; then for a, b != a
    and c of `cuts`, in lexicographic order, the one-point crossover PlanCross(a, b, c, 26): a's years before c, b's from c on."""
    cuts = [int(c) for c in cuts]
    return [PlanCross(p, p, 0, 0) for p in range(n_plans)] + \
           [PlanCross(a, b, c, N.YEARS) for a in range(n_plans) for b in range(n_plans) if b != a for c in cuts]


def _objective_mask(objectives, who: str) -> int:
    mask = 0
    for name in objectives:
        if name not in PARETO_OBJECTIVES:
            raise ValueError(f"{who}: unknown objective {name!r} (one of {', '.join(PARETO_OBJECTIVES)})")
        mask |= 1 << PARETO_OBJECTIVES.index(name)
    return mask


def _archive_mode(cost_only: bool, keep: str, who: str) -> int:
    """The `mode` of an archive: the rank score (1 | 2) and the capacity rule, "score" or "spread" (EG_PARETO_KEEP_SPREAD)."""
    if keep not in ("score", "spread"):
        raise ValueError(f"{who}: keep = {keep!r} (\"score\" or \"spread\")")
    return (2 if cost_only else 1) | (N.PARETO_KEEP_SPREAD if keep == "spread" else 0)


def pareto_filter(front_index, front_metrics, index, metrics, status, mask: int):
    """One step of a streaming non-dominated filter on the host, with eg_pareto_track's definitions over the objectives of `mask` (bit
    i = metric i): an entry is valid with status EG_EP_OK and none of its four metrics NaN; a dominates b when it is at least as good
    in every active metric (lower emissions and cost, higher opinion and reliability) and strictly better in one; entries whose
    active metrics are all equal are one point, held once by the entry that came first.  (front_index [f], front_metrics [f,4]): a
    front in ascending index; the entries (index [n] ascending and above the front's, metrics [n,4], status [n]) are taken in in
    order.  Returns the new (front_index, front_metrics), ascending."""
    active = [i for i in range(4) if mask >> i & 1]
    sign = np.array([1.0, -1.0, 1.0, -1.0])[active]      # (as costs: lower is better)
    fi = [int(i) for i in front_index]
    fm = np.asarray(front_metrics, np.float64).reshape(-1, 4)
    fg = fm[:, active] * sign
    metrics = np.asarray(metrics, np.float64).reshape(-1, 4)
    valid = (np.asarray(status) == N.EG_EP_OK) & ~np.isnan(metrics).any(axis=1)
    for j in np.flatnonzero(valid):
        g = metrics[j, active] * sign
        if len(fi) and (fg <= g).all(axis=1).any():      # dominated by a held point, or the same point
            continue
        keep = ~(g <= fg).all(axis=1)                    # (none of them equals g: what g is at least as good as, it dominates)
        fi = [i for i, k in zip(fi, keep) if k] + [int(index[j])]
        fm = np.concatenate([fm[keep], metrics[j:j + 1]]); fg = np.concatenate([fg[keep], g[None]])
    return np.array(fi, np.int64), fm


@dataclass
class CrossFront:
    """Engine.cross_front: the non-dominated variants among the parents and their one-cut children, a row each in ascending variant
    number — the variant's number in cross_pairs' order, its PlanCross, its four metrics, its rank score and whether it is a parent."""
    variant: np.ndarray       # [k]
    crosses: list             # [k] PlanCross
    metrics: np.ndarray       # [k,4]
    score: np.ndarray         # [k]
    is_parent: np.ndarray     # [k] bool
    n_variants: int           # variants evaluated
    n_valid: int              # ... of which valid


BREED_STOP = ("converged", "max_generations", "empty")      # EG_BREED_*


def _cross_name(parents, x) -> str:
    """a variant's name as scripts/cross_front.py writes it: a parent keeps its own, a child is `A>B@year`, the year being the first
    one taken from B (a plan without a name goes by its position in the population)"""
    if x.a == x.b or x.from_year == x.to_year:
        return parents[x.a].name
    name = lambda p: parents[p].name or str(p)
    return f"{name(x.a)}>{name(x.b)}@{2025 + x.from_year}"


@dataclass(frozen=True)
class BreedGeneration:
    """One generation of Engine.breed_front (eg_breed_generation): the population it started from, the crosses left out because a
    child would outgrow a list, what was evaluated and valid, what the archive kept (and how many of those are children) and dropped
    for want of room."""
    n_parents: int
    n_skipped: int
    n_kept: int
    n_children_kept: int
    n_variants: int
    n_valid: int
    n_dropped: int


@dataclass(frozen=True)
class BreedMember:
    """A survivor of a generation (eg_breed_member): its PlanCross against that generation's population, its variant number, rank
    score and four metrics."""
    cross: PlanCross
    variant: int
    score: float
    metrics: tuple


@dataclass
class BreedFront:
    """Engine.breed_front: the final population (plans, a row of metrics and a rank score each, in ascending variant number of the last
    generation), a BreedGeneration per generation that ran, every generation's survivors ([generation][member] BreedMember — the whole
    genealogy), why it stopped (one of BREED_STOP) and the final members' records (a BatchResult; None after "empty")."""
    plans: list
    metrics: np.ndarray       # [k,4]
    score: np.ndarray         # [k]
    generations: list
    members: list
    stop_reason: str
    records: "BatchResult" = None

    def lineage(self, parents) -> "list[list[Plan]]":
        """Every population from P_0 = `parents` on, rebuilt on the host from the genealogy: P_{g+1} is members[g]'s crosses applied to
        P_g (PlanCross.apply), named as scripts/cross_front.py names them.  A generation that kept nothing leaves the population as it
        was.  lineage(parents)[-1] is what `plans` holds."""
        pops = [[Plan(p.best_actions, p.best_deficit_actions, p.name) for p in parents]]
        for kept in self.members:
            if not kept:
                break
            pop = pops[-1]
            nxt = []
            for m in kept:
                child = m.cross.apply(pop)
                nxt.append(Plan(child.best_actions, child.best_deficit_actions, _cross_name(pop, m.cross)))
            pops.append(nxt)
        return pops


EXPLORE_STOP = ("explored", "max_generations", "empty", "budget")      # EG_EXPLORE_*


@dataclass(frozen=True)
class ExploreGeneration:
    """One generation of Engine.explore_front (eg_explore_generation): the frontier whose neighbourhoods it evaluated, what the archive
    held after it and how many of those entered in it (the next frontier), the generation's variants and how many were valid, and
    what the archive has dropped for want of room so far."""
    n_frontier: int
    n_held: int
    n_new: int
    n_variants: int
    n_valid: int
    n_dropped: int


@dataclass(frozen=True)
class ExploreMember:
    """A member of a frontier (eg_explore_member): the number of the plan it was made from (-1: a start plan), the PlanEdit or PlanMove
    against that plan (a start plan: PlanEdit()), its own number, rank score and four metrics."""
    parent: int
    edit: object
    number: int
    score: float
    metrics: tuple


def _explore_name(parent_name: str, parent: int, edit) -> str:
    """a neighbour's name: its base's (a plan without a name goes by its number), then what was done to it, e.g. `A-2031.2`, `A~2031.2=17`,
    `A+2040=9`, `A:2031.2>2033` (best_deficit_actions: `d` in front of the year)"""
    base = parent_name or str(parent)
    if isinstance(edit, PlanMove):
        return f"{base}:{2025 + edit.year}.{edit.pos}>{2025 + edit.to_year}"
    at = f"{'d' if edit.list else ''}{2025 + edit.year}"
    if edit.kind == "delete":
        return f"{base}-{at}.{edit.pos}"
    if edit.kind == "replace":
        return f"{base}~{at}.{edit.pos}={edit.action}"
    if edit.kind == "insert":
        return f"{base}+{at}={edit.action}"
    return parent_name


@dataclass
class ExploreFront:
    """Engine.explore_front: the final population — the whole archive: plans, their numbers, a row of metrics and a rank score each, in
    ascending number —, an ExploreGeneration per generation that ran, the members ([0]: the start plans held after generation 0;
    [g + 1]: the frontier F_{g+1}, the members that entered in generation g — the whole genealogy), why it stopped (one of
    EXPLORE_STOP) and the final members' records (a BatchResult; None after "empty")."""
    plans: list
    numbers: np.ndarray       # [k]
    metrics: np.ndarray       # [k,4]
    score: np.ndarray         # [k]
    generations: list
    members: list
    stop_reason: str
    records: "BatchResult" = None

    def lineage(self, starts) -> "list[dict]":
        """Every frontier's plans, rebuilt on the host from the genealogy: element g of the list is {number: Plan} of everything known
        after row g of `members` — the start plans (numbers 0..n-1), then every member with its edit or move applied to its parent's
        plan (PlanEdit.apply, PlanMove.apply) and named after it.  Frontier g is the entries of element g whose numbers stand in
        members[g]; lineage(starts)[-1] filtered to `numbers` is what `plans` holds."""
        known = {p: Plan(s.best_actions, s.best_deficit_actions, s.name) for p, s in enumerate(starts)}
        out = []
        for row in self.members:
            for m in row:
                if m.parent < 0:
                    continue
                base = known[m.parent]
                child = m.edit.apply(base)
                known[m.number] = Plan(child.best_actions, child.best_deficit_actions, _explore_name(base.name, m.parent, m.edit))
            out.append(dict(known))
        return out


@dataclass
class Timing:
    """Engine.plan_timing: per move (row 0: the base plan, as the move of an entry onto itself, or None for a plan without entries) the
    record's status, the four metrics, the rank score (NaN for a variant that failed) and their differences from row 0 (NaN where the
    base or the variant failed): the rows Sensitivity has for edits."""
    moves: list
    result: "BatchResult"
    status: np.ndarray        # [n]
    metrics: np.ndarray       # [n,4]
    score: np.ndarray         # [n]
    d_metrics: np.ndarray     # [n,4]
    d_score: np.ndarray       # [n]


def _edit_array(edits):
    edits = list(edits)
    arr = (N.EgPlanEdit * max(len(edits), 1))()
    for j, e in enumerate(edits):
        arr[j] = e.struct() if isinstance(e, PlanEdit) else e
    return arr, len(edits)


@dataclass
class Sensitivity:
    """Engine.plan_sensitivity: per edit (row 0: the base plan) the record's status, the four metrics, the rank score (NaN for a variant
    that failed) and their differences from row 0 (NaN where the base or the variant failed)."""
    edits: list
    result: "BatchResult"
    status: np.ndarray        # [n]
    metrics: np.ndarray       # [n,4]
    score: np.ndarray         # [n]
    d_metrics: np.ndarray     # [n,4]
    d_score: np.ndarray       # [n]


def sensitivity_edits(base: "Plan", replace_with=None) -> "list[PlanEdit]":
    """The canonical edit order of a sensitivity run: the base itself; every best_actions entry in (year, position) order as a delete;
    every best_deficit_actions entry likewise; then, per best_actions entry, a replace by each action of `replace_with`."""
    edits = [PlanEdit()]
    for which, lists in enumerate((base.best_actions, base.best_deficit_actions)):
        edits += [PlanEdit("delete", which, y, i) for y, l in enumerate(lists) for i in range(len(l))]
    for a in (replace_with or ()):
        assert 0 <= int(a) < N.N_ACTIONS, a
    edits += [PlanEdit("replace", 0, y, i, int(a)) for y, l in enumerate(base.best_actions) for i in range(len(l)) for a in (replace_with or ())]
    return edits


def refine_edits(base: "Plan", replace_with=None, append_with=None) -> "list[PlanEdit]":
    """The variants of one round of Engine.refine_plan, in order: sensitivity_edits(base, replace_with), then per year and action of
    `append_with` that action appended to the year's best_actions list — no appends while best_actions holds 4 096 entries."""
    edits = sensitivity_edits(base, replace_with)
    for a in (append_with or ()):
        assert 0 <= int(a) < N.N_ACTIONS, a
    if len(base) < N.RUN_CAP:
        edits += [PlanEdit("insert", 0, y, len(l), int(a)) for y, l in enumerate(base.best_actions) for a in (append_with or ())]
    return edits


@dataclass
class RefineStep:
    """One applied edit of Engine.refine_plan (eg_refine_step): the edit against the plan of its round, its place among the round's
    n_variants variants, how many of them were no candidates, and the score and metrics it reached."""
    edit: "PlanEdit"      # (a PlanMove where the step is a move: Engine.refine_plans with max_shift > 0)
    variant: int
    n_variants: int
    n_failed: int
    score: float
    metrics: np.ndarray


REFINE_STOP = ("local_optimum", "max_rounds", "base_failed")


def _refine_steps(steps) -> "list[RefineStep]":
    """eg_refine_step structs as RefineSteps"""
    return [RefineStep(PlanEdit(PlanEdit.KINDS[s.edit.kind], s.edit.list, s.edit.year, s.edit.pos, s.edit.action), s.variant, s.n_variants, s.n_failed,
                       s.score, np.array(s.metrics[:])) for s in steps]


def _refine_move_steps(steps) -> "list[RefineStep]":
    """eg_refine_move_step structs as RefineSteps, the move where the step is one"""
    return [RefineStep(PlanMove(s.move.list, s.move.year, s.move.pos, s.move.to_year, s.move.to_pos) if s.is_move else
                       PlanEdit(PlanEdit.KINDS[s.edit.kind], s.edit.list, s.edit.year, s.edit.pos, s.edit.action), s.variant, s.n_variants, s.n_failed,
                       s.score, np.array(s.metrics[:])) for s in steps]


@dataclass
class RepairStep:
    """One applied edit or move of Engine.repair_plans (eg_repair_step): the edit (a PlanMove where the step is a move) against the plan of
    its round, its place among the round's n_variants variants, how many of them were no candidates and how many candidates were feasible,
    and the mask of violated constraints, the violation measure V, the score and the metrics it reached."""
    edit: "PlanEdit"
    variant: int
    n_variants: int
    n_failed: int
    n_feasible: int
    violated: int
    violation: float
    score: float
    metrics: np.ndarray


REPAIR_STOP = ("feasible", "max_rounds", "base_failed", "stuck")


def _repair_steps(steps) -> "list[RepairStep]":
    """eg_repair_step structs as RepairSteps, the move where the step is one"""
    return [RepairStep(PlanMove(s.move.list, s.move.year, s.move.pos, s.move.to_year, s.move.to_pos) if s.is_move else
                       PlanEdit(PlanEdit.KINDS[s.edit.kind], s.edit.list, s.edit.year, s.edit.pos, s.edit.action), s.variant, s.n_variants, s.n_failed,
                       s.n_feasible, int(s.violated), s.violation, s.score, np.array(s.metrics[:])) for s in steps]


def _refine_opts(mode, max_rounds, replace_with, append_with):
    """(eg_refine_opts, the arrays it points into)"""
    rep = np.array(list(replace_with or []), np.uint8); app = np.array(list(append_with or []), np.uint8)
    opts = N.EgRefineOpts(int(mode), int(max_rounds), len(rep), _p(rep, C.c_uint8) if len(rep) else None, len(app), _p(app, C.c_uint8) if len(app) else None)
    return opts, (rep, app)


PARETO_OBJECTIVES = ("emissions", "opinion", "cost", "reliability")      # bit i of eg_pareto_track's mask = metric i


def _fetch_top_k(fn, handle, what):
    """(BatchResult of the n_held entries in rank order, scores [n_held], global indices [n_held]) of a top-K archive."""
    res = BatchResult.alloc(N.TOPK_MAX)
    out = res.struct()
    held = C.c_int32(0)
    scores = np.zeros(N.TOPK_MAX); index = np.zeros(N.TOPK_MAX, np.int64)
    N.check(fn(handle, C.byref(out), C.byref(held), _p(scores, C.c_double), _p(index, C.c_int64)), what)
    n = held.value
    rows = BatchResult(*[np.ascontiguousarray(getattr(res, f.name)[:n]) for f in fields(BatchResult)])
    return rows, scores[:n].copy(), index[:n].copy()


@dataclass
class BatchResult:
    metrics: np.ndarray       # [n,4] final_net_emissions, average_public_opinion, total_cost, power_reliability
    yearly: np.ndarray        # [n,26,21]
    status: np.ndarray
    n_run: np.ndarray; n_def: np.ndarray; n_act: np.ndarray
    run_log: np.ndarray; def_log: np.ndarray; act_log: np.ndarray
    n_gens: np.ndarray; gen_cell: np.ndarray; gen_pack: np.ndarray
    n_offsets: np.ndarray; off_pack: np.ndarray
    n_draws: np.ndarray; bytes_moved: np.ndarray
    n_chunks: np.ndarray = None      # [n] chunks of 64 candidate records the searches requested (see include/eirgrid_hip.h)

    @staticmethod
    def alloc(n: int) -> "BatchResult":
        z = np.zeros
        return BatchResult(z((n, 4)), z((n, N.YEARS, N.YEARLY_FIELDS)), z(n, np.int32), z((n, N.YEARS), np.int32),
                           z((n, N.YEARS), np.int32), z((n, N.YEARS), np.int32), z((n, N.RUN_CAP), np.uint8),
                           z((n, N.DEF_CAP), np.uint8), z((n, N.ACT_CAP), np.uint8), z(n, np.int32),
                           z((n, N.MAX_GENS), np.uint16), z((n, N.MAX_GENS), np.uint16), z(n, np.int32),
                           z((n, N.MAX_OFFSETS), np.uint16), z(n, np.uint64), z(n), z(n, np.uint32))

    def struct(self) -> N.EgEpisodeOut:
        return N.EgEpisodeOut(_p(self.metrics, C.c_double), _p(self.yearly, C.c_double), _p(self.status, C.c_int32),
                              _p(self.n_run, C.c_int32), _p(self.n_def, C.c_int32), _p(self.n_act, C.c_int32),
                              _p(self.run_log, C.c_uint8), _p(self.def_log, C.c_uint8), _p(self.act_log, C.c_uint8),
                              _p(self.n_gens, C.c_int32), _p(self.gen_cell, C.c_uint16), _p(self.gen_pack, C.c_uint16),
                              _p(self.n_offsets, C.c_int32), _p(self.off_pack, C.c_uint16), _p(self.n_draws, C.c_uint64),
                              _p(self.bytes_moved, C.c_double), _p(self.n_chunks, C.c_uint32))

    def export_summary_csv(self, path: str, timestamp: str = "", episode: int = 0) -> None:
        """simulation_summary.csv (utils/csv_export.rs:215-432) of one episode of this result."""
        one = BatchResult(*[np.ascontiguousarray(getattr(self, f)[episode:episode + 1]) for f in
                            ("metrics", "yearly", "status", "n_run", "n_def", "n_act", "run_log", "def_log", "act_log", "n_gens",
                             "gen_cell", "gen_pack", "n_offsets", "off_pack", "n_draws", "bytes_moved", "n_chunks")])
        out = one.struct()
        N.check(N.lib().eg_export_summary_csv(C.byref(out), path.encode(), timestamp.encode()), "eg_export_summary_csv")

    def export_run_details(self, world: World, out_dir: str, settlement_names=None, offset_seed: int = 0, episode: int = 0) -> None:
        """yearly_details/{settlements,generators,carbon_offsets}.csv + operation_logs/generator_operation_logs.csv of one
        episode of this result (utils/csv_export.rs:434-1230; eg_export_run_details)."""
        one = BatchResult(*[np.ascontiguousarray(getattr(self, f)[episode:episode + 1]) for f in
                            ("metrics", "yearly", "status", "n_run", "n_def", "n_act", "run_log", "def_log", "act_log", "n_gens",
                             "gen_cell", "gen_pack", "n_offsets", "off_pack", "n_draws", "bytes_moved", "n_chunks")])
        out = one.struct()
        w, keep = _world_struct(world)
        names = None
        if settlement_names is not None:
            names = (C.c_char_p * len(settlement_names))(*[n.encode() for n in settlement_names])
        N.check(N.lib().eg_export_run_details(C.byref(w), names, C.byref(out), str(out_dir).encode(), C.c_uint64(offset_seed & (2**64 - 1))),
                "eg_export_run_details")

    def bytes_touched(self) -> np.ndarray:
        """Per episode: the SURVEY §8(d) bytes with the score field of every search (2601 x 8 B, never read by the
        branch-and-bound search) replaced by the candidate records the search requested (n_chunks x 64 x 32 B)."""
        return self.bytes_moved - self.n_gens.astype(np.float64) * (N.CELLS * 8.0) + self.n_chunks.astype(np.float64) * (64 * 32.0)

    def bytes_requested(self) -> np.ndarray:
        """Per episode: the bytes the kernel REQUESTS from the memory system (L2 or HBM), by construction of the code — without
        the SURVEY formula's state term `2 (59 + G) 56` per year (state that lives in LDS: 3 bytes per generator) and without the
        generator coordinates a search reads (LDS as well):
          n_chunks x 2048                       sorted candidate records in chunks of 64 x 32 B; long-replay episodes: + the entries of
                                                their penalty field they gather and update (counted by the kernel)
          32 x sum_g (25 - b_g)                 year-start gathers per generator and later year: {cost, cost opinion} 16 B, m03 8 B, t12 8 B
          16 x sum_o (25 - b_o)                 per carbon offset and later year: tonnes 8 B, cost 8 B
          32 x n_gens + 24 x n_offsets          the terms of an addition itself
          26 x 1024                             the policy row block of every year (128 doubles)
          26 x 168 + 3 x 104 + 72               stores: yearly rows, per-year counts, record header
          2 x (run + def) + act + 4 x n_gens + 2 x n_offsets    stores: logs (run and def re-read by the statistics epilogue), placements"""
        n = len(self.status)
        out = np.zeros(n)
        for e in range(n):
            g, o = int(self.n_gens[e]), int(self.n_offsets[e])
            by = (self.gen_pack[e, :g].astype(np.int64) >> 4) & 31
            oy = (self.off_pack[e, :o].astype(np.int64) >> 4) & 31
            logs = 2.0 * (self.n_run[e].sum() + self.n_def[e].sum()) + self.n_act[e].sum()
            out[e] = (self.n_chunks[e] * 2048.0 + 32.0 * (25 - by).sum() + 16.0 * (25 - oy).sum() + 32.0 * g + 24.0 * o + 26 * 1024.0
                      + 26 * 168.0 + 3 * 104.0 + 72.0 + logs + 4.0 * g + 2.0 * o)
        return out

    def lists(self, e: int, which: str):
        log = {"run": self.run_log, "def": self.def_log, "act": self.act_log}[which][e]
        cnt = {"run": self.n_run, "def": self.n_def, "act": self.n_act}[which][e]
        out, pos = [], 0
        for c in cnt:
            out.append(log[pos:pos + c].tolist()); pos += int(c)
        return out


class Engine:
    """One eg_ctx: a world resident in the HBM of one MI355X."""

    def __init__(self, world: World, device: int = 0):
        L = N.lib()
        if L.eg_device_count() <= 0:
            raise N.EirgridError("no HIP device visible: eirgrid_amd runs on MI355X (gfx950) only and has no CPU path")
        w, self._keep = _world_struct(world)
        self.h = L.eg_create(device, C.byref(w))
        if not self.h:
            raise N.EirgridError(L.eg_last_error().decode())
        self.world = world

    def close(self):
        if getattr(self, "h", None):
            try:
                N.lib().eg_destroy(self.h)
            except TypeError:      # interpreter shutdown: module globals are already gone
                pass
            self.h = None

    __del__ = close

    @staticmethod
    def _opts(enable_energy_sales=True, enable_construction_delays=False, write_yearly=True):
        return N.EgOpts(int(enable_energy_sales), int(enable_construction_delays), int(write_yearly))

    def rollout_batch(self, weights: ActionWeights, seed: int, n_episodes: int, first_episode_index: int = 0,
                      replay_mask=None, enable_energy_sales=True, enable_construction_delays=False,
                      write_yearly=True, out: "BatchResult" = None) -> BatchResult:
        """Batched `run_iteration` (core/iteration.rs:10-20): episodes first..first+n against one weights snapshot.
        `out`: a BatchResult of the same size to fill again (a caller in a loop keeps its buffers; list entries behind an episode's
        counts keep whatever they held)."""
        res = out if out is not None else BatchResult.alloc(n_episodes)
        assert res.status.shape == (n_episodes,)
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, enable_construction_delays, write_yearly)
        mask = None
        if replay_mask is not None:
            self._mask = np.ascontiguousarray(replay_mask, dtype=np.uint8)
            assert self._mask.shape == (n_episodes,)
            mask = _p(self._mask, C.c_uint8)
        out = res.struct()
        N.check(N.lib().eg_rollout_batch(self.h, C.byref(snap), C.byref(opts), C.c_uint64(seed & (2**64 - 1)),
                                         C.c_uint64(first_episode_index), n_episodes, mask, C.byref(out)), "eg_rollout_batch")
        return res

    def run_iteration(self, iteration: int, weights: ActionWeights, replay_best_strategy: bool, seed: int,
                      enable_energy_sales: bool = True, enable_construction_delays: bool = False) -> BatchResult:
        """Single-episode form with the reference's argument order (core/iteration.rs:10-20)."""
        mask = np.array([1 if replay_best_strategy else 0], dtype=np.uint8)
        return self.rollout_batch(weights, seed, 1, iteration, mask, enable_energy_sales, enable_construction_delays)

    def evaluate_plans(self, weights: ActionWeights, plans, seed: int, first_episode_index: int = 0, enable_energy_sales=True,
                       write_yearly=True) -> BatchResult:
        """Score given plans (eg_evaluate_plans): plan j is the replay episode at global index first_episode_index + j under `weights`,
        with has_best = 1 and the plan as its best lists.  Trains nothing and leaves the resident policy alone; rank the results with
        rank_score(res.metrics[j], cost_only)."""
        ps = plans if isinstance(plans, PlanSet) else PlanSet(plans)
        res = BatchResult.alloc(ps.s.n_plans)
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        N.check(N.lib().eg_evaluate_plans(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.c_uint64(seed & (2**64 - 1)),
                                          C.c_uint64(first_episode_index), C.byref(out)), "eg_evaluate_plans")
        return res

    def set_constraints(self, constraints) -> None:
        """Plan constraints (eg_plan_constraints_set): a list of Constraint (or specs for Constraint.parse), at most 32; an empty list
        clears them.  They hold for every later plan batch of this engine — evaluate_plans / _plan_edits / _plan_moves / _plan_crosses /
        _plan_rewrites, refine_plan(s), breed_front, explore_front, cross_front, technology_report, plan_timing, plan_sensitivity: a variant
        that ended EG_EP_OK and violates one comes back with status EG_EP_INFEASIBLE (metrics and rows untouched), and every search skips
        it as it skips a failed variant.  So: refining an infeasible base stops with "base_failed"; a step's n_failed counts the
        infeasible variants; explore_front from infeasible starts admits their feasible neighbours; repair_plans descends on the violation
        itself, the directed way to repair a plan.  Training
        batches (rollout_batch, device_step, ...) are never judged.  While row constraints are set the plan calls refuse write_yearly=False.
        The list may hold BuildConstraints (specs with "built(": bounds on what an episode builds, eg_build_constraints_set) BEHIND the row
        constraints, together at most 32: mask bits, excess columns and repair weights follow the list's order, so a row constraint behind
        a build constraint raises ValueError."""
        rows, builds = split_constraints(constraints)      # (walked and parsed once: a generator is fine)
        L = N.lib()
        # checked before anything is cleared, so a list that is refused leaves what was set: the row setter's own refusal, as ever
        arr, n = constraint_array(rows)
        if L.eg_plan_constraints_validate(arr, n) != N.EG_OK:
            N.check(L.eg_plan_constraints_set(self.h, arr, n), "eg_plan_constraints_set")
        barr, nb = build_constraint_array(builds)
        N.check(L.eg_build_constraints_validate(barr, nb), "eg_build_constraints_validate")
        # both kinds cleared first, so neither setter meets the other kind's old count
        N.check(L.eg_plan_constraints_set(self.h, None, 0), "eg_plan_constraints_set")
        N.check(L.eg_build_constraints_set(self.h, None, 0), "eg_build_constraints_set")
        self._constraints = []
        N.check(L.eg_plan_constraints_set(self.h, arr, n), "eg_plan_constraints_set")
        self._constraints = rows
        N.check(L.eg_build_constraints_set(self.h, barr, nb), "eg_build_constraints_set")
        self._constraints = rows + builds

    def clear_constraints(self) -> None:
        self.set_constraints([])

    def last_batch_constraints(self) -> "list[Constraint | BuildConstraint]":
        """The constraints the LAST batch was judged under (eg_last_batch_constraints, then eg_last_batch_build_constraints: the row
        constraints, then the build constraints) — not those set now; [] when it was not judged."""
        arr = (N.EgPlanConstraint * N.CONSTRAINTS_MAX)()
        k = N.lib().eg_last_batch_constraints(self.h, arr)
        N.check(min(k, 0), "eg_last_batch_constraints")
        barr = (N.EgBuildConstraint * N.CONSTRAINTS_MAX)()
        kb = N.lib().eg_last_batch_build_constraints(self.h, barr)
        N.check(min(kb, 0), "eg_last_batch_build_constraints")
        return [Constraint._from_struct(arr[i]) for i in range(k)] + [BuildConstraint._from_struct(barr[i]) for i in range(kb)]

    def fetch_feasibility(self):
        """(violated [n] uint32, excess [n, k] float64) of the last plan batch (eg_fetch_plan_feasibility): bit i of violated[j] is set iff
        variant j violates constraint i of last_batch_constraints() — the k constraints that were set when the batch ran, whatever has
        been set or cleared since; excess[j, i] <= 0 means satisfied, its negative is the slack, NaN violates.  A variant that failed on
        its own has mask 0 and a row of NaN.  Refused when the last batch ran without constraints."""
        L = N.lib()
        n = int(L.eg_last_batch_size(self.h))
        k = int(L.eg_last_batch_constraints(self.h, None)) + int(L.eg_last_batch_build_constraints(self.h, None))      # rows, then builds
        if k <= 0 or n == 0:      # the library's own refusal, nothing written
            N.check(L.eg_fetch_plan_feasibility(self.h, None, None), "eg_fetch_plan_feasibility")
            raise N.EirgridError("eg_fetch_plan_feasibility: the last batch ran without plan constraints")
        violated, excess = np.zeros(n, np.uint32), np.zeros((n, k), np.float64)
        N.check(L.eg_fetch_plan_feasibility(self.h, _p(violated, C.c_uint32), _p(excess, C.c_double)), "eg_fetch_plan_feasibility")
        return violated, excess

    def set_streams(self, n: int, tail=None, cost_only: bool = False) -> None:
        """Plan streams (eg_plan_streams_set): every later plan batch of this engine runs n passes, pass r the batch as it runs without
        streams at its first index + r, and comes back with stream 0's episode in the records — rows, lists, the feasibility masks — but
        COMMITTED metrics and status: the mean of the `tail` worst streams by rank_score(., cost_only) (tail=None: all n, the mean
        outcome; tail=1: the worst stream's metrics), and the first stream's status that is not EG_EP_OK.  evaluate_plans / _plan_edits /
        _plan_moves / _plan_crosses / _plan_rewrites, refine_plan(s), cross_front, breed_front, explore_front, technology_report,
        plan_timing, plan_sensitivity, plan_feasibility and fold_pareto_last_batch then work on committed outcomes; repair_plans is
        refused while streams are set.  n 0 or 1 clears the setting.  Training batches never see it."""
        n = int(n)
        N.check(N.lib().eg_plan_streams_set(self.h, n, n if tail is None else int(tail), 2 if cost_only else 1), "eg_plan_streams_set")

    def clear_streams(self) -> None:
        N.check(N.lib().eg_plan_streams_set(self.h, 0, 0, 0), "eg_plan_streams_set")

    def last_batch_streams(self):
        """(n, tail, cost_only) the LAST batch ran under (eg_last_batch_streams) — not what is set now; n is 0 when it ran without streams."""
        tail, mode = C.c_int32(0), C.c_int32(0)
        n = N.lib().eg_last_batch_streams(self.h, C.byref(tail), C.byref(mode))
        N.check(min(n, 0), "eg_last_batch_streams")
        return n, tail.value, mode.value == 2

    def fetch_ensemble(self) -> Ensemble:
        """The eg_ensemble_row of every variant of the last batch (eg_fetch_plan_ensemble); refused when it ran without streams."""
        L = N.lib()
        n = int(L.eg_last_batch_size(self.h))
        rows = (N.EgEnsembleRow * max(n, 1))()
        N.check(L.eg_fetch_plan_ensemble(self.h, rows), "eg_fetch_plan_ensemble")
        a = np.frombuffer(rows, dtype=np.dtype([("nominal", "<f8", 4), ("committed", "<f8", 4), ("score_min", "<f8"), ("score_max", "<f8"), ("score_sum", "<f8"),
                                                ("n_ok", "<i4"), ("n_infeasible", "<i4"), ("n_failed", "<i4"), ("worst_stream", "<i4"), ("status", "<i4"),
                                                ("pad", "<i4", 5)]))[:n]
        return Ensemble(*[a[f.name].copy() for f in fields(Ensemble)])

    def fetch_streams(self):
        """(metrics [R, n, 4], status [R, n]) of every stream of the last batch (eg_fetch_plan_streams): what pass r left in the records,
        stream 0's being what the batch would hold without streams; refused when it ran without streams."""
        L = N.lib()
        n, R = int(L.eg_last_batch_size(self.h)), int(L.eg_last_batch_streams(self.h, None, None))
        if R <= 0 or n == 0:      # the library's own refusal, nothing written
            N.check(L.eg_fetch_plan_streams(self.h, None, None), "eg_fetch_plan_streams")
            raise N.EirgridError("eg_fetch_plan_streams: the last batch ran without plan streams")
        metrics, status = np.zeros((R, n, 4), np.float64), np.zeros((R, n), np.int32)
        N.check(L.eg_fetch_plan_streams(self.h, _p(metrics, C.c_double), _p(status, C.c_int32)), "eg_fetch_plan_streams")
        return metrics, status

    def plan_feasibility(self, weights: ActionWeights, plans, seed: int, index: int = 0, constraints=None):
        """Which of `plans` satisfy which constraints: evaluates them as evaluate_plans does (plan j at global index index + j) under
        `constraints` (None: the ones that are set) and returns (status [n], violated: per plan the list of the violated Constraints,
        excess [n, k]; a negative excess is the slack).  The engine's own constraints are as before afterwards.
        Under set_streams the status is the committed one — infeasible as soon as one stream violates a constraint — while the violated
        lists and the excess rows are stream 0's: fetch_ensemble().n_infeasible tells in how many streams a plan was infeasible."""
        before = list(getattr(self, "_constraints", ()))
        if constraints is not None:
            self.set_constraints(constraints)
        try:
            if not getattr(self, "_constraints", ()):
                raise ValueError("plan_feasibility: no constraints given and none set")
            res = self.evaluate_plans(weights, plans, seed, index)
            cs = self.last_batch_constraints()
            mask, excess = self.fetch_feasibility()
        finally:
            if constraints is not None:
                self.set_constraints(before)
        return res.status.copy(), [[c for i, c in enumerate(cs) if (int(m) >> i) & 1] for m in mask], excess

    def evaluate_plan_edits(self, weights: ActionWeights, base: "Plan", edits, seed: int, first_index: int = 0, same_index: bool = True,
                            enable_energy_sales=True, write_yearly=True) -> BatchResult:
        """Score edits of one plan (eg_evaluate_plan_edits): variant j is `base` with edits[j] (PlanEdit) applied, evaluated as
        evaluate_plans would evaluate it — at global index first_index for every variant (same_index: the same fallback draws), or at
        first_index + j.  The variants' plan blocks are built on the device."""
        ps = PlanSet([base])
        arr, n = _edit_array(edits)
        res = BatchResult.alloc(max(n, 1))
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        N.check(N.lib().eg_evaluate_plan_edits(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), arr, n, C.c_uint64(seed & (2**64 - 1)),
                                               C.c_uint64(first_index), int(bool(same_index)), C.byref(out)), "eg_evaluate_plan_edits")
        return res

    def evaluate_plan_moves(self, weights: ActionWeights, base: "Plan", moves, seed: int, first_index: int = 0, same_index: bool = True,
                            enable_energy_sales=True, write_yearly=True) -> BatchResult:
        """Score moves of one plan (eg_evaluate_plan_moves): variant j is `base` with moves[j] (PlanMove) applied, evaluated as
        evaluate_plans would evaluate it — at global index first_index for every variant (same_index), or at first_index + j.  The
        variants' plan blocks are built on the device."""
        ps = PlanSet([base])
        arr, n = _move_array(moves)
        res = BatchResult.alloc(max(n, 1))
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        N.check(N.lib().eg_evaluate_plan_moves(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), arr, n, C.c_uint64(seed & (2**64 - 1)),
                                               C.c_uint64(first_index), int(bool(same_index)), C.byref(out)), "eg_evaluate_plan_moves")
        return res

    def evaluate_plan_crosses(self, weights: ActionWeights, parents, crosses, seed: int, first_index: int = 0, same_index: bool = True,
                              enable_energy_sales=True, write_yearly=True) -> BatchResult:
        """Score crosses of a set of parent plans (eg_evaluate_plan_crosses): variant j is crosses[j] (PlanCross) applied to `parents`,
        evaluated as evaluate_plans would evaluate it — at global index first_index for every variant (same_index), or at
        first_index + j.  The variants' plan blocks are built on the device."""
        ps = parents if isinstance(parents, PlanSet) else PlanSet(parents)
        arr, n = _cross_array(crosses)
        res = BatchResult.alloc(max(n, 1))
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        N.check(N.lib().eg_evaluate_plan_crosses(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), arr, n, C.c_uint64(seed & (2**64 - 1)),
                                                 C.c_uint64(first_index), int(bool(same_index)), C.byref(out)), "eg_evaluate_plan_crosses")
        return res

    def cross_front(self, weights: ActionWeights, parents, seed: int, index: int = 0, objectives=PARETO_OBJECTIVES, cost_only: bool = False,
                    cuts=range(1, 26), max_variants: int = N.CROSS_MAX_VARIANTS) -> CrossFront:
        """The non-dominated plans among `parents` and their one-cut children: the variants of cross_pairs(len(parents), cuts), evaluated
        in chunks of at most max_variants (<= 16 384) in order, every one at global index `index` of `seed` (the same fallback draws),
        and filtered on the host with eg_pareto_track's definitions over `objectives` (pareto_filter), chunk by chunk against the
        front so far; an equal point is held once, at the lowest variant number.  Per variant only the metrics and the status come
        back (36 bytes).  The context's own Pareto archive is not touched.  cost_only picks the rank score of the rows.
        Under set_streams every variant is judged over the R streams: the metrics, statuses and scores here are the committed ones."""
        mask = _objective_mask(objectives, "cross_front")
        if mask == 0:
            raise ValueError("cross_front: no objectives")
        if not 1 <= int(max_variants) <= N.CROSS_MAX_VARIANTS:
            raise ValueError(f"cross_front: max_variants = {max_variants} (1..{N.CROSS_MAX_VARIANTS})")
        parents = list(parents)
        ps = PlanSet(parents)
        crosses = cross_pairs(len(parents), cuts)
        snap = weights.snapshot()
        opts = self._opts(True, False, False)      # (no yearly rows: nothing reads them)
        L = N.lib()
        fi, fm = np.zeros(0, np.int64), np.zeros((0, 4))
        n_valid = 0
        for first in range(0, len(crosses), int(max_variants)):
            arr, n = _cross_array(crosses[first:first + int(max_variants)])
            N.check(L.eg_evaluate_plan_crosses(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), arr, n, C.c_uint64(seed & (2**64 - 1)),
                                               C.c_uint64(index), 1, None), "eg_evaluate_plan_crosses")
            metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32)
            out = N.EgEpisodeOut(metrics=_p(metrics, C.c_double), status=_p(status, C.c_int32))
            N.check(L.eg_fetch(self.h, C.byref(out)), "eg_fetch")
            n_valid += int(((status == N.EG_EP_OK) & ~np.isnan(metrics).any(axis=1)).sum())
            fi, fm = pareto_filter(fi, fm, np.arange(first, first + n), metrics, status, mask)
        score = np.array([rank_score(m, cost_only) for m in fm])
        return CrossFront(fi, [crosses[i] for i in fi], fm, score, fi < len(parents), len(crosses), n_valid)

    def evaluate_plan_rewrites(self, weights: ActionWeights, plans, maps, rewrites, seed: int, first_index: int = 0, same_index: bool = True,
                               enable_energy_sales=True, write_yearly=True) -> BatchResult:
        """Score rewrites of a set of plans (eg_evaluate_plan_rewrites): variant j is rewrites[j] (PlanRewrite) applied to `plans` and
        `maps` (ActionMap), evaluated as evaluate_plans would evaluate it — at global index first_index for every variant (same_index),
        or at first_index + j.  The variants' plan blocks are built on the device."""
        ps = plans if isinstance(plans, PlanSet) else PlanSet(plans)
        marr, n_maps = _map_array(maps)
        arr, n = _rewrite_array(rewrites)
        res = BatchResult.alloc(max(n, 1))
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        N.check(N.lib().eg_evaluate_plan_rewrites(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), marr, n_maps, arr, n, C.c_uint64(seed & (2**64 - 1)),
                                                  C.c_uint64(first_index), int(bool(same_index)), C.byref(out)), "eg_evaluate_plan_rewrites")
        return res

    def technology_report(self, weights: ActionWeights, plans, seed: int, index: int = 0, cost_only: bool = False, deficit: str = "substitute",
                          substitute_with: int = 3 * 12, max_variants: int = N.REWRITE_MAX_VARIANTS) -> "list[TechnologyRow]":
        """What every generator type is worth to every plan: the variants of technology_rewrites(plans, deficit, substitute_with) — per
        plan the plan itself, then the plan without each type t its best_actions uses: t dropped there and, with deficit ==
        "substitute", replaced by `substitute_with` (battery storage at 100 %) in best_deficit_actions, where a dropped entry would be
        refilled by fallback draws; deficit == "keep" leaves that list alone — evaluated in chunks of at most max_variants (<= 16 384)
        in order, every one at global index `index` of `seed`.  Per variant only the metrics and the status come back (36 bytes); a
        plan whose deficit list holds the type taken out goes up once more with that list substituted (technology_rewrites).
        The context's own Pareto archive is not touched.  Rows in the variants' order; cost_only picks the rank score.
        Under set_streams every variant is judged over the R streams: the metrics, statuses and scores here are the committed ones."""
        if not 1 <= int(max_variants) <= N.REWRITE_MAX_VARIANTS:
            raise ValueError(f"technology_report: max_variants = {max_variants} (1..{N.REWRITE_MAX_VARIANTS})")
        plans = list(plans)
        parents, maps, rewrites, rows = technology_rewrites(plans, deficit, substitute_with)
        marr, n_maps = _map_array(maps)
        snap = weights.snapshot()
        opts = self._opts(True, False, False)      # (no yearly rows: nothing reads them)
        L = N.lib()
        metrics = np.zeros((len(rewrites), 4)); status = np.zeros(len(rewrites), np.int32)
        first = 0
        while first < len(rewrites):
            # a chunk: at most max_variants variants over at most CROSS_MAX_PARENTS of the parents, renumbered for the chunk's set
            local, chunk = {}, []
            for r in rewrites[first:first + int(max_variants)]:
                if r.plan not in local and len(local) == N.CROSS_MAX_PARENTS:
                    break
                chunk.append(PlanRewrite(local.setdefault(r.plan, len(local)), r.map, r.from_year, r.to_year, r.lists))
            ps = PlanSet([parents[p] for p in local])
            arr, n = _rewrite_array(chunk)
            N.check(L.eg_evaluate_plan_rewrites(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), marr, n_maps, arr, n, C.c_uint64(seed & (2**64 - 1)),
                                                C.c_uint64(index), 1, None), "eg_evaluate_plan_rewrites")
            m, st = metrics[first:first + n], status[first:first + n]
            out = N.EgEpisodeOut(metrics=_p(m, C.c_double), status=_p(st, C.c_int32))
            N.check(L.eg_fetch(self.h, C.byref(out)), "eg_fetch")
            first += n
        report, own = [], 0.0
        for j, (p, t, removed) in enumerate(rows):
            score = rank_score(metrics[j], cost_only)
            if t < 0:
                own = score
            report.append(TechnologyRow(p, t, removed, int(status[j]), tuple(float(v) for v in metrics[j]), score, score - own))
        return report

    def breed_front(self, weights: ActionWeights, parents, seed: int, index: int = 0, objectives=PARETO_OBJECTIVES, cost_only: bool = False,
                    cuts=range(1, 26), generations: int = 8, cap: int = N.PARETO_MAX, max_variants: int = N.CROSS_MAX_VARIANTS,
                    keep: str = "score") -> BreedFront:
        """Generations of cross_front on the device (eg_breed_plans): from the population `parents`, every generation evaluates the
        variants of cross_pairs(len(population), cuts) — less the crosses whose child would outgrow a list — in chunks of at most
        max_variants, every one at global index `index` of `seed`, folds each chunk into a private Pareto archive of `cap` entries
        over `objectives` (eg_pareto_track's rules; cost_only picks the rank score the capacity rule and the rows use, `keep` the
        capacity rule: "score" keeps the best-scoring points of a front larger than cap, "spread" a spread-out subset), and makes the
        survivors' plan blocks the next population without leaving the device.  Stops when a generation keeps exactly its parents, after
        `generations` generations, or when nothing was valid.  The context's own Pareto archive is not touched."""
        mask, mode = _objective_mask(objectives, "breed_front"), _archive_mode(cost_only, keep, "breed_front")
        if mask == 0:
            raise ValueError("breed_front: no objectives")
        parents = list(parents)
        ps = PlanSet(parents)
        cut = np.array([int(c) for c in cuts], np.int64)
        if len(cut) == 0 or (cut < 0).any() or (cut > 255).any():      # (what a byte cannot carry; eg_breed_validate checks the rest)
            raise ValueError(f"breed_front: cuts = {cut.tolist()} (year indices 1..{N.YEARS - 1}, at least one)")
        cut = cut.astype(np.uint8)
        gens, cap = int(generations), int(cap)
        bo = N.EgBreedOpts(mode, mask, cap, gens, len(cut), _p(cut, C.c_uint8), int(max_variants))
        L = N.lib()
        N.check(L.eg_breed_validate(C.byref(ps.s), C.byref(bo)), "eg_breed_validate")
        rows = (N.EgBreedGeneration * gens)()
        members = (N.EgBreedMember * (gens * cap))()
        n_gen, stop = C.c_int32(0), C.c_int32(0)
        population = C.POINTER(N.EgPlanSet)()
        res = BatchResult.alloc(cap)
        snap = weights.snapshot()
        opts = self._opts(True, False, True)
        out = res.struct()
        N.check(L.eg_breed_plans(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(bo), C.c_uint64(seed & (2**64 - 1)), C.c_uint64(index),
                                 C.byref(population), rows, members, C.byref(n_gen), C.byref(stop), C.byref(out)), "eg_breed_plans")
        plans = Plan._take_set(population)
        reason = BREED_STOP[stop.value]
        g_rows = [BreedGeneration(*(int(getattr(rows[g], f)) for f, _ in N.EgBreedGeneration._fields_)) for g in range(n_gen.value)]
        kept = [[BreedMember(PlanCross(m.cross.a, m.cross.b, m.cross.from_year, m.cross.to_year), int(m.variant), float(m.score), tuple(m.metrics))
                 for m in members[g * cap:g * cap + g_rows[g].n_kept]] for g in range(n_gen.value)]
        front = BreedFront(plans, np.zeros((0, 4)), np.zeros(0), g_rows, kept, reason, None)
        if reason != "empty":
            last = kept[-1]
            front.metrics = np.array([m.metrics for m in last], np.float64).reshape(-1, 4)
            front.score = np.array([m.score for m in last], np.float64)
            names = [f.name for f in fields(BatchResult)]
            front.records = BatchResult(*[np.ascontiguousarray(getattr(res, f)[:len(last)]) for f in names])
            for plan, named in zip(plans, front.lineage(parents)[-1]):
                plan.name = named.name
        else:
            for plan, p in zip(plans, parents):
                plan.name = p.name
        return front

    def explore_front(self, weights: ActionWeights, starts, seed: int, index: int = 0, objectives=PARETO_OBJECTIVES, cost_only: bool = False,
                      generations: int = 8, cap: int = N.PARETO_MAX, replace_with=None, append_with=None, max_shift: int = 0,
                      max_variants: int = 0, launch: int = 0, keep: str = "score") -> ExploreFront:
        """A Pareto local search over one-entry edits and moves on the device (eg_explore_plans): generation 0 evaluates the plans of
        `starts` and their neighbourhoods — refine_edits(plan, replace_with, append_with)[1:] + refine_moves(plan, max_shift) —, every
        later generation the neighbourhoods of the members that entered the archive in the one before, every variant at global index
        `index` of `seed` in chunks of `launch` (0: 16 384), each chunk folded into ONE private Pareto archive of `cap` entries over
        `objectives` that lives through the call (eg_pareto_track's rules; cost_only picks the rank score the capacity rule and the
        rows use, `keep` the capacity rule: "score" or "spread", as for breed_front).  Stops when no member is left unexplored, when nothing was valid, when the next generation would take the call
        beyond max_variants (0: no budget) or after `generations` generations.  The context's own Pareto archive is not touched."""
        mask, mode = _objective_mask(objectives, "explore_front"), _archive_mode(cost_only, keep, "explore_front")
        if mask == 0:
            raise ValueError("explore_front: no objectives")
        starts = list(starts)
        ps = PlanSet(starts)
        rep = np.array([int(a) for a in (replace_with or [])], np.int64); app = np.array([int(a) for a in (append_with or [])], np.int64)
        for name, l in (("replace_with", rep), ("append_with", app)):
            if ((l < 0) | (l > 255)).any():      # (what a byte cannot carry; eg_explore_validate checks the rest)
                raise ValueError(f"explore_front: {name} = {l.tolist()} (actions 0..{N.N_ACTIONS - 1})")
        rep, app = rep.astype(np.uint8), app.astype(np.uint8)
        gens, cap = int(generations), int(cap)
        xo = N.EgExploreOpts(mode, mask, cap, gens, len(rep), _p(rep, C.c_uint8) if len(rep) else None, len(app),
                             _p(app, C.c_uint8) if len(app) else None, int(max_shift), int(launch), int(max_variants))
        L = N.lib()
        N.check(L.eg_explore_validate(C.byref(ps.s), C.byref(xo)), "eg_explore_validate")
        rows = (N.EgExploreGeneration * gens)()
        members = (N.EgExploreMember * ((gens + 1) * cap))()
        numbers = (C.c_int64 * cap)()
        n_gen, stop = C.c_int32(0), C.c_int32(0)
        population = C.POINTER(N.EgPlanSet)()
        res = BatchResult.alloc(cap)
        snap = weights.snapshot()
        opts = self._opts(True, False, True)
        out = res.struct()
        N.check(L.eg_explore_plans(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(xo), C.c_uint64(seed & (2**64 - 1)), C.c_uint64(index),
                                   C.byref(population), rows, members, numbers, C.byref(n_gen), C.byref(stop), C.byref(out)), "eg_explore_plans")
        plans = Plan._take_set(population)
        reason = EXPLORE_STOP[stop.value]
        fields_g = ("n_frontier", "n_held", "n_new", "n_variants", "n_valid", "n_dropped")
        g_rows = [ExploreGeneration(*(int(getattr(rows[g], f)) for f in fields_g)) for g in range(n_gen.value)]

        def member(m):
            edit = PlanMove(m.move.list, m.move.year, m.move.pos, m.move.to_year, m.move.to_pos) if m.is_move else \
                PlanEdit(PlanEdit.KINDS[m.edit.kind], m.edit.list, m.edit.year, m.edit.pos, m.edit.action)
            return ExploreMember(int(m.parent), edit, int(m.number), float(m.score), tuple(m.metrics))
        kept = []
        if reason != "empty":
            # row 0: the start plans held after generation 0 — what generation 0 held less what entered as a neighbour
            kept.append([member(m) for m in members[:g_rows[0].n_held - g_rows[0].n_new]])
            kept += [[member(m) for m in members[(g + 1) * cap:(g + 1) * cap + g_rows[g].n_new]] for g in range(n_gen.value)]
        front = ExploreFront(plans, np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros(0), g_rows, kept, reason, None)
        if reason != "empty":
            front.numbers = np.array(numbers[:len(plans)], np.int64)
            by_number = {m.number: m for row in kept for m in row}
            last = [by_number[int(k)] for k in front.numbers]
            front.metrics = np.array([m.metrics for m in last], np.float64).reshape(-1, 4)
            front.score = np.array([m.score for m in last], np.float64)
            names = [f.name for f in fields(BatchResult)]
            front.records = BatchResult(*[np.ascontiguousarray(getattr(res, f)[:len(last)]) for f in names])
            line = front.lineage(starts)[-1]
            for plan, k in zip(plans, front.numbers):
                plan.name = line[int(k)].name
        else:
            for plan, p in zip(plans, starts):
                plan.name = p.name
        return front

    def plan_timing(self, weights: ActionWeights, base: "Plan", seed: int, mode: int = 1, max_shift: int = 1) -> Timing:
        """Which entries of `base` would be better placed in another year: the base (row 0) and the moves of refine_moves(base,
        max_shift) in one batch, all at global index 0 of `seed`; per move the metrics, eg_rank_score in `mode` (1: optimization_mode
        None, 2: cost_only) and their differences from the base's.
        Under set_streams every variant is judged over the R streams: the metrics, statuses and scores here are the committed ones."""
        moves = refine_moves(base, max_shift)
        first = next(((y, 0) for y, l in enumerate(base.best_actions) if l), None)
        if first is None:      # nothing to move: the base alone, through the plan batch
            res = self.evaluate_plans(weights, [base], seed, 0)
            rows = [None]
        else:
            rows = [PlanMove(0, first[0], 0, first[0], 0)] + moves      # (an entry moved onto itself: the base)
            res = self.evaluate_plan_moves(weights, base, rows, seed, 0, True)
        L = N.lib()
        score = np.array([L.eg_rank_score(_p(np.ascontiguousarray(res.metrics[j]), C.c_double), int(mode)) if res.status[j] == N.EG_EP_OK else np.nan
                          for j in range(len(rows))])
        both = (res.status == N.EG_EP_OK) & (res.status[0] == N.EG_EP_OK)
        d_metrics = np.where(both[:, None], res.metrics - res.metrics[0], np.nan)
        return Timing(rows, res, res.status.copy(), res.metrics.copy(), score, d_metrics, np.where(both, score - score[0], np.nan))

    def debug_fetch_plan_block(self, plan: int) -> np.ndarray:
        """Test hook (eg_debug_fetch_plan_block): the bytes of plan block `plan` of the last plan or plan-edit batch."""
        out = np.zeros(N.PLAN_BLOCK_BYTES, np.uint8)
        N.check(N.lib().eg_debug_fetch_plan_block(self.h, int(plan), _p(out, C.c_uint8)), "eg_debug_fetch_plan_block")
        return out

    def plan_sensitivity(self, weights: ActionWeights, base: "Plan", seed: int, mode: int = 1, replace_with=None) -> Sensitivity:
        """Which actions of `base` matter: the edits of sensitivity_edits(base, replace_with), all at global index 0 of `seed`; per edit
        the metrics, eg_rank_score in `mode` (1: optimization_mode None, 2: cost_only) and their differences from the base's.
        Under set_streams every variant is judged over the R streams: the metrics, statuses and scores here are the committed ones."""
        edits = sensitivity_edits(base, replace_with)
        res = self.evaluate_plan_edits(weights, base, edits, seed, 0, True)
        L = N.lib()
        score = np.array([L.eg_rank_score(_p(np.ascontiguousarray(res.metrics[j]), C.c_double), int(mode)) if res.status[j] == N.EG_EP_OK else np.nan
                          for j in range(len(edits))])
        # (differences are NaN where the base or the variant failed, as the CLI writes them)
        both = (res.status == N.EG_EP_OK) & (res.status[0] == N.EG_EP_OK)
        d_metrics = np.where(both[:, None], res.metrics - res.metrics[0], np.nan)
        return Sensitivity(edits, res, res.status.copy(), res.metrics.copy(), score, d_metrics, np.where(both, score - score[0], np.nan))

    def refine_plan(self, weights: ActionWeights, base: "Plan", seed: int, index: int = 0, mode: int = 1, max_rounds: int = 64, replace_with=None,
                    append_with=None, enable_energy_sales=True, write_yearly=True):
        """Greedy refinement of `base` on the device (eg_refine_plan): per round the variants of refine_edits(plan, replace_with,
        append_with), all at global index `index` of `seed`; the best candidate by eg_rank_score in `mode` (ties: the lowest variant, so
        only a strict improvement moves the plan) becomes the next round's plan.  Returns (refined Plan, [RefineStep], stop reason — one of
        REFINE_STOP —, the base's score (NaN when it failed), the refined plan's record as a BatchResult of one episode, or None when the
        base failed)."""
        ps = PlanSet([base])
        ro, keep = _refine_opts(mode, max_rounds, replace_with, append_with)
        steps = (N.EgRefineStep * max(int(max_rounds), 1))()
        n_steps, stop = C.c_int32(0), C.c_int32(0)
        start = C.c_double(float("nan"))
        refined = C.POINTER(N.EgPlanSet)()
        res = BatchResult.alloc(1)
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        L = N.lib()
        N.check(L.eg_refine_plan(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(ro), C.c_uint64(seed & (2**64 - 1)), C.c_uint64(index),
                                 C.byref(refined), steps, C.byref(n_steps), C.byref(stop), C.byref(start), C.byref(out)), "eg_refine_plan")
        plan = Plan._take_set(refined)[0]
        reason = REFINE_STOP[stop.value]
        return plan, _refine_steps(steps[:n_steps.value]), reason, start.value, (None if reason == "base_failed" else res)

    def refine_plans(self, weights: ActionWeights, bases, seed: int, index: int = 0, mode: int = 1, max_rounds: int = 64, replace_with=None,
                     append_with=None, enable_energy_sales=True, write_yearly=True, max_shift: int = 0):
        """Greedy refinement of many plans in one call (eg_refine_plans): the rounds of all plans stepped together, a launch holding the
        variants of as many plans as fit.  Returns a list with one tuple per plan of `bases` (1..REFINE_MAX_PLANS plans), each exactly the
        tuple refine_plan returns for that plan alone.
        max_shift > 0 (eg_refine_plans_moves): behind a round's edits come the moves of refine_moves(plan, max_shift), a best_actions
        entry shifted by up to max_shift years; a step that is a move carries a PlanMove as its `edit`."""
        ps = bases if isinstance(bases, PlanSet) else PlanSet(bases)
        n = ps.s.n_plans
        ro, keep = _refine_opts(mode, max_rounds, replace_with, append_with)
        rounds = max(int(max_rounds), 1)
        moves = int(max_shift) != 0
        steps = ((N.EgRefineMoveStep if moves else N.EgRefineStep) * (max(n, 1) * rounds))()
        n_steps = np.zeros(max(n, 1), np.int32); stop = np.zeros(max(n, 1), np.int32)
        start = np.full(max(n, 1), np.nan)
        refined = C.POINTER(N.EgPlanSet)()
        res = BatchResult.alloc(max(n, 1))
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        out = res.struct()
        L = N.lib()
        if moves:
            mo = N.EgRefineMoveOpts(int(max_shift))
            N.check(L.eg_refine_plans_moves(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(ro), C.byref(mo), C.c_uint64(seed & (2**64 - 1)),
                                            C.c_uint64(index), C.byref(refined), steps, _p(n_steps, C.c_int32), _p(stop, C.c_int32), _p(start, C.c_double),
                                            C.byref(out)), "eg_refine_plans_moves")
        else:
            N.check(L.eg_refine_plans(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(ro), C.c_uint64(seed & (2**64 - 1)), C.c_uint64(index),
                                      C.byref(refined), steps, _p(n_steps, C.c_int32), _p(stop, C.c_int32), _p(start, C.c_double), C.byref(out)), "eg_refine_plans")
        plans = Plan._take_set(refined)
        names = [f.name for f in fields(BatchResult)]
        result = []
        for p in range(n):
            reason = REFINE_STOP[int(stop[p])]
            rec = None if reason == "base_failed" else BatchResult(*[np.ascontiguousarray(getattr(res, f)[p:p + 1]) for f in names])
            result.append((plans[p], (_refine_move_steps if moves else _refine_steps)(steps[p * rounds:p * rounds + int(n_steps[p])]), reason, float(start[p]), rec))
        return result

    def repair_plans(self, weights: ActionWeights, bases, seed: int, index: int = 0, mode: int = 1, max_rounds: int = 64, replace_with=None,
                     append_with=None, max_shift: int = 0, violation_weights=None, enable_energy_sales=True):
        """Greedy descent on the violation of the engine's constraints (eg_repair_plans; set_constraints first): per round the variants of
        refine_plans(..., max_shift) for every plan of `bases` (1..REFINE_MAX_PLANS plans), of which the candidate with the smallest
        violation measure V below the plan's own — constraints.violation of its excess row under `violation_weights`, one per constraint,
        None: 1.0 each; ties to the largest eg_rank_score in `mode`, then to the lowest variant — becomes the plan, until V is 0.  Returns
        one tuple per plan: (plan, [RepairStep], stop reason — one of REPAIR_STOP —, the base's V (NaN when it failed), the returned plan's
        V, its record as a BatchResult of one episode, or None when the base failed)."""
        ps = bases if isinstance(bases, PlanSet) else PlanSet(bases)
        n = ps.s.n_plans
        ro, keep = _refine_opts(mode, max_rounds, replace_with, append_with)
        rounds = max(int(max_rounds), 1)
        mo = N.EgRefineMoveOpts(int(max_shift))
        vw = None if violation_weights is None else np.ascontiguousarray(list(violation_weights), dtype=np.float64)
        k = len(getattr(self, "_constraints", ()))
        if vw is not None and k and len(vw) != k:      # (none set: the library's own refusal)
            raise ValueError(f"{len(vw)} violation weights for {k} constraints")
        steps = (N.EgRepairStep * (max(n, 1) * rounds))()
        n_steps = np.zeros(max(n, 1), np.int32); stop = np.zeros(max(n, 1), np.int32)
        start = np.full(max(n, 1), np.nan); final = np.full(max(n, 1), np.nan)
        repaired = C.POINTER(N.EgPlanSet)()
        res = BatchResult.alloc(max(n, 1))
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, True)
        out = res.struct()
        N.check(N.lib().eg_repair_plans(self.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(ro), C.byref(mo) if int(max_shift) != 0 else None,
                                        None if vw is None else _p(vw, C.c_double), C.c_uint64(seed & (2**64 - 1)), C.c_uint64(index), C.byref(repaired), steps,
                                        _p(n_steps, C.c_int32), _p(stop, C.c_int32), _p(start, C.c_double), _p(final, C.c_double), C.byref(out)), "eg_repair_plans")
        plans = Plan._take_set(repaired)
        names = [f.name for f in fields(BatchResult)]
        result = []
        for p in range(n):
            reason = REPAIR_STOP[int(stop[p])]
            rec = None if reason == "base_failed" else BatchResult(*[np.ascontiguousarray(getattr(res, f)[p:p + 1]) for f in names])
            result.append((plans[p], _repair_steps(steps[p * rounds:p * rounds + int(n_steps[p])]), reason, float(start[p]), float(final[p]), rec))
        return result

    # device-resident path used by bench.py
    def upload_snapshot(self, weights: ActionWeights, enable_energy_sales=True, write_yearly=True):
        snap = weights.snapshot()
        opts = self._opts(enable_energy_sales, False, write_yearly)
        N.check(N.lib().eg_upload_snapshot(self.h, C.byref(snap), C.byref(opts)), "eg_upload_snapshot")

    def launch(self, seed: int, first_episode_index: int, n_episodes: int, replay_mask=None):
        mask = None
        if replay_mask is not None:
            self._mask = np.ascontiguousarray(replay_mask, dtype=np.uint8)
            mask = _p(self._mask, C.c_uint8)
        N.check(N.lib().eg_rollout_launch(self.h, C.c_uint64(seed & (2**64 - 1)), C.c_uint64(first_episode_index),
                                          n_episodes, mask), "eg_rollout_launch")

    def launch_update(self, seed: int, first_episode_index: int, n_episodes: int, d_packet_ptr: int, replay_mask=None):
        """Fused step: rollout + update statistics + best-candidate pick into a PACKET_BYTES device buffer."""
        mask = None
        if replay_mask is not None:
            self._mask = np.ascontiguousarray(replay_mask, dtype=np.uint8)
            mask = _p(self._mask, C.c_uint8)
        N.check(N.lib().eg_rollout_launch_update(self.h, C.c_uint64(seed & (2**64 - 1)), C.c_uint64(first_episode_index),
                                                 n_episodes, mask, C.c_void_p(d_packet_ptr)), "eg_rollout_launch_update")

    def train_step(self, weights: ActionWeights, seed: int, first_episode_index: int, n_episodes: int, replay_mask=None,
                   noise_seed: int = 0, enable_energy_sales=True, write_yearly=True) -> bool:
        """eg_train_step: the whole single-GPU training step in one library call.  Returns True on a new best strategy."""
        mask = None
        if replay_mask is not None:
            self._mask = np.ascontiguousarray(replay_mask, dtype=np.uint8)
            mask = _p(self._mask, C.c_uint8)
        opts = self._opts(enable_energy_sales, False, write_yearly)
        rc = N.lib().eg_train_step(self.h, weights.h, C.byref(opts), C.c_uint64(seed & (2**64 - 1)), C.c_uint64(first_episode_index),
                                   n_episodes, mask, C.c_uint64(noise_seed & (2**64 - 1)))
        if rc < 0:
            N.check(rc, "eg_train_step")
        return rc == 1

    # ---- device-resident policy (include/eirgrid_hip.h: eg_policy_push ... eg_policy_pull) ----
    def push(self, weights: ActionWeights, enable_energy_sales=True, write_yearly=True):
        opts = self._opts(enable_energy_sales, False, write_yearly)
        N.check(N.lib().eg_policy_push(self.h, weights.h, C.byref(opts)), "eg_policy_push")

    def device_rollout(self, seed: int, first_episode_index: int, n_episodes: int, replay_period: int, d_packet_ptr: int):
        N.check(N.lib().eg_device_rollout(self.h, C.c_uint64(seed & (2**64 - 1)), C.c_uint64(first_episode_index), n_episodes,
                                          replay_period, C.c_void_p(d_packet_ptr)), "eg_device_rollout")

    def device_apply(self, d_packets_ptr: int, n_packets: int, d_own_packet_ptr: int, noise_seed: int):
        N.check(N.lib().eg_device_apply(self.h, C.c_void_p(d_packets_ptr), n_packets, C.c_void_p(d_own_packet_ptr),
                                        C.c_uint64(noise_seed & (2**64 - 1))), "eg_device_apply")

    def device_step(self, seed: int, first_episode_index: int, n_episodes: int, replay_period: int, noise_seed: int):
        N.check(N.lib().eg_device_step(self.h, C.c_uint64(seed & (2**64 - 1)), C.c_uint64(first_episode_index), n_episodes,
                                       replay_period, C.c_uint64(noise_seed & (2**64 - 1))), "eg_device_step")

    def hold(self):
        """Keep a device-side copy of the device-resident policy (eg_policy_hold)."""
        N.check(N.lib().eg_policy_hold(self.h), "eg_policy_hold")

    def rewind(self):
        """Put the held copy back (eg_policy_rewind)."""
        N.check(N.lib().eg_policy_rewind(self.h), "eg_policy_rewind")

    def replay_hoist(self, on: bool = True) -> None:
        """Compute the replay episodes of every batch once instead of once per episode (eg_replay_hoist; include/eirgrid_hip.h)."""
        N.check(N.lib().eg_replay_hoist(self.h, int(bool(on))), "eg_replay_hoist")

    def replay_hoist_stats(self):
        """(batches launched with the hoist armed, whether the last of them was served by it).  Synchronises."""
        n, last = C.c_uint64(), C.c_int32()
        N.check(N.lib().eg_replay_hoist_stats(self.h, C.byref(n), C.byref(last)), "eg_replay_hoist_stats")
        return int(n.value), bool(last.value)

    def pull(self, weights: ActionWeights):
        N.check(N.lib().eg_policy_pull(self.h, weights.h), "eg_policy_pull")

    def sync(self):
        N.check(N.lib().eg_sync(self.h), "eg_sync")

    def fetch(self, n_episodes: int = None) -> BatchResult:
        """Every output of the last launched batch (eg_fetch copies eg_last_batch_size() records)."""
        last = int(N.lib().eg_last_batch_size(self.h))
        if n_episodes is not None and n_episodes != last:
            raise ValueError(f"fetch({n_episodes}): the last launched batch holds {last} episodes")
        res = BatchResult.alloc(last)
        out = res.struct()
        N.check(N.lib().eg_fetch(self.h, C.byref(out)), "eg_fetch")
        return res

    def timing_reset(self):
        N.check(N.lib().eg_timing_reset(self.h))

    def timing_read(self):
        ms, n = C.c_double(), C.c_int32()
        N.check(N.lib().eg_timing_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def memory_report(self):
        """{tables, records, field_pool} in bytes of device memory (eg_memory_report)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        N.check(N.lib().eg_memory_report(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"tables": a.value, "records": b.value, "field_pool": c.value}

    def timing_read_grids(self):
        """(span ms, sum of the grids' own ms, launches): grids of a batch that ran side by side show span < sum."""
        span, grids, n = C.c_double(), C.c_double(), C.c_int32()
        N.check(N.lib().eg_timing_read_grids(self.h, C.byref(span), C.byref(grids), C.byref(n)))
        return span.value, grids.value, n.value

    def update_stats(self, d_stats_ptr: int):
        """Reduce the last launched batch into an int64[STATS_LEN] DEVICE buffer (e.g. torch tensor .data_ptr())."""
        N.check(N.lib().eg_update_stats(self.h, C.c_void_p(d_stats_ptr)), "eg_update_stats")

    def fetch_record(self, episode: int) -> BatchResult:
        """Every output of one episode of the last batch, as a one-episode BatchResult."""
        res = BatchResult.alloc(1)
        out = res.struct()
        N.check(N.lib().eg_fetch_record(self.h, episode, C.byref(out)), "eg_fetch_record")
        return res

    def fetch_best_run(self):
        """(state, record): the record of the episode that is the policy's best strategy (strategy.rs:19-258), kept by the
        on-device update.  state 0 = no improvement yet, 1 = record valid, 2 = it ran on another rank.  (The run the reference
        exports is another one: fetch_best_result.)"""
        res = BatchResult.alloc(1)
        out = res.struct()
        state = C.c_int32(0)
        N.check(N.lib().eg_fetch_best_run(self.h, C.byref(out), C.byref(state)), "eg_fetch_best_run")
        return state.value, (res if state.value == 1 else None)

    def track_best_result(self, cost_only: bool = False, on: bool = True) -> None:
        """Start the reference's `best_result` fold at None (core/multi_simulation.rs:384, :613-620): every batch launched from
        now on is folded on the device in iteration order (eg_best_result_track)."""
        N.check(N.lib().eg_best_result_track(self.h, 0 if not on else (2 if cost_only else 1)), "eg_best_result_track")

    def fetch_best_result(self):
        """(global index, record) of the run the reference would summarise and export, or (None, None) before any result."""
        res = BatchResult.alloc(1)
        out = res.struct()
        state = C.c_int32(0); index = C.c_int64(-1)
        N.check(N.lib().eg_fetch_best_result(self.h, C.byref(out), C.byref(state), C.byref(index)), "eg_fetch_best_result")
        return (int(index.value), res) if state.value == 1 else (None, None)

    def track_top_k(self, k: int, cost_only: bool = False) -> None:
        """Start an empty top-K archive of the k best distinct scenarios (eg_top_k_track); every batch launched from now on is folded
        into it on the device.  k = 0 stops tracking (the archive stays fetchable)."""
        N.check(N.lib().eg_top_k_track(self.h, int(k), 0 if k == 0 else (2 if cost_only else 1)), "eg_top_k_track")

    def fetch_top_k(self):
        """(BatchResult of the n_held entries in rank order, their rank scores, their global indices)."""
        return _fetch_top_k(N.lib().eg_fetch_top_k, self.h, "eg_fetch_top_k")

    def track_pareto(self, cap: int, objectives=PARETO_OBJECTIVES, cost_only: bool = False, keep: str = "score") -> None:
        """Start an empty Pareto archive of at most `cap` non-dominated outcomes over the named objectives (eg_pareto_track); every
        training batch launched from now on is folded into it on the device.  cap = 0 stops tracking (the archive stays fetchable).
        When the front outgrows cap, `keep` decides what stays: "score" the points of the largest rank score (cost_only picks the score),
        "spread" a farthest-point selection on the normalised front, which starts from the best-scoring point."""
        mask = _objective_mask(objectives, "track_pareto")
        N.check(N.lib().eg_pareto_track(self.h, int(cap), mask, _archive_mode(cost_only, keep, "track_pareto")), "eg_pareto_track")

    def fetch_pareto(self):
        """(BatchResult of the n_held entries in ascending global index, their global indices, their rank scores, n_dropped)."""
        L = N.lib()
        held = C.c_int32(0); dropped = C.c_int64(0)
        N.check(L.eg_fetch_pareto(self.h, None, C.byref(held), None, None, None), "eg_fetch_pareto")
        n = held.value      # (nothing folds between the two calls: rows for the held entries only, not for EG_PARETO_MAX)
        res = BatchResult.alloc(max(n, 1))
        out = res.struct()
        scores = np.zeros(max(n, 1)); index = np.zeros(max(n, 1), np.int64)
        N.check(L.eg_fetch_pareto(self.h, C.byref(out), C.byref(held), _p(index, C.c_int64), _p(scores, C.c_double), C.byref(dropped)), "eg_fetch_pareto")
        assert held.value == n
        rows = BatchResult(*[np.ascontiguousarray(getattr(res, f.name)[:n]) for f in fields(BatchResult)])
        return rows, index[:n].copy(), scores[:n].copy(), int(dropped.value)

    def fold_pareto_last_batch(self) -> None:
        """Fold the last batch — whatever kind it was, a plan batch included — into the Pareto archive (eg_pareto_fold_last_batch)."""
        N.check(N.lib().eg_pareto_fold_last_batch(self.h), "eg_pareto_fold_last_batch")

    def _debug_pareto_fold(self, metrics, status, first_index: int) -> None:
        """Test hook (eg_debug_pareto_fold): a batch of synthetic records with these metrics [n,4] and status [n], folded."""
        m = np.ascontiguousarray(metrics, dtype=np.float64).reshape(-1, 4)
        st = np.ascontiguousarray(status, dtype=np.int32)
        assert len(st) == len(m)
        N.check(N.lib().eg_debug_pareto_fold(self.h, _p(m, C.c_double), _p(st, C.c_int32), len(m), C.c_uint64(int(first_index))), "eg_debug_pareto_fold")

    def _debug_load_batch(self, metrics, status, first_index: int, n_act=None, act_log=None, score_list=None) -> None:
        """Test hook (eg_debug_load_batch): the record buffer becomes a batch of synthetic records with these metrics [n,4] and status [n],
        tagged with their global index; optionally n_act [n,26], whole act_log rows [n,ACT_CAP] and the score list [n]."""
        m = np.ascontiguousarray(metrics, dtype=np.float64).reshape(-1, 4)
        st = np.ascontiguousarray(status, dtype=np.int32)
        n = len(m)
        assert st.shape == (n,)
        na = al = sl = None
        if n_act is not None:
            na = np.ascontiguousarray(n_act, dtype=np.int32); assert na.shape == (n, N.YEARS)
        if act_log is not None:
            al = np.ascontiguousarray(act_log, dtype=np.uint8); assert al.shape == (n, N.ACT_CAP)
        if score_list is not None:
            sl = np.ascontiguousarray(score_list, dtype=np.float64); assert sl.shape == (n,)
        N.check(N.lib().eg_debug_load_batch(self.h, _p(m, C.c_double), _p(st, C.c_int32), None if na is None else _p(na, C.c_int32),
                                            None if al is None else _p(al, C.c_uint8), None if sl is None else _p(sl, C.c_double), n,
                                            C.c_uint64(int(first_index))), "eg_debug_load_batch")

    def _debug_load_built(self, n_gens, gen_pack, n_offsets, off_pack) -> None:
        """Test hook (eg_debug_load_built): the counts [n] and the whole lists [n,4096] (uint16) of what the records of the crafted batch
        _debug_load_batch made built — what lies behind the counts goes up too."""
        ng, no = np.ascontiguousarray(n_gens, dtype=np.int32), np.ascontiguousarray(n_offsets, dtype=np.int32)
        gp, op = np.ascontiguousarray(gen_pack, dtype=np.uint16), np.ascontiguousarray(off_pack, dtype=np.uint16)
        assert gp.shape == (len(ng), N.MAX_GENS) and op.shape == (len(no), N.MAX_OFFSETS) and len(ng) == len(no)
        N.check(N.lib().eg_debug_load_built(self.h, _p(ng, C.c_int32), _p(gp, C.c_uint16), _p(no, C.c_int32), _p(op, C.c_uint16), len(ng)), "eg_debug_load_built")

    def _debug_load_yearly(self, yearly) -> None:
        """Test hook (eg_debug_load_yearly): the yearly rows [n,26,21] of the crafted batch _debug_load_batch made."""
        y = np.ascontiguousarray(yearly, dtype=np.float64).reshape(-1, N.YEARS, N.YEARLY_FIELDS)
        N.check(N.lib().eg_debug_load_yearly(self.h, _p(y, C.c_double), len(y)), "eg_debug_load_yearly")

    def _debug_constrain_last_batch(self) -> None:
        """Test hook (eg_debug_constrain_last_batch): k_plan_constraints — with a build constraint set, k_build_constraints — over the last
        batch, as a plan batch ends."""
        N.check(N.lib().eg_debug_constrain_last_batch(self.h), "eg_debug_constrain_last_batch")

    def _debug_ensemble_keep(self, r: int) -> None:
        """Test hook (eg_debug_ensemble_keep): k_ensemble_keep over the last batch's records, into slab r of the store."""
        N.check(N.lib().eg_debug_ensemble_keep(self.h, int(r)), "eg_debug_ensemble_keep")

    def _debug_ensemble_commit(self, n_streams: int, tail: int, cost_only: bool = False) -> None:
        """Test hook (eg_debug_ensemble_commit): k_ensemble_commit over slabs 0..n_streams-1 and the last batch's records."""
        N.check(N.lib().eg_debug_ensemble_commit(self.h, int(n_streams), int(tail), 2 if cost_only else 1), "eg_debug_ensemble_commit")

    def _debug_fold_last_batch(self, best_result: bool = False, top_k: bool = False, use_score_list: bool = False) -> None:
        """Test hook (eg_debug_fold_last_batch): what a training batch runs behind its rollout for the chosen folds, on the last batch."""
        what = (N.DEBUG_FOLD_BEST_RESULT if best_result else 0) | (N.DEBUG_FOLD_TOP_K if top_k else 0)
        N.check(N.lib().eg_debug_fold_last_batch(self.h, what, int(use_score_list)), "eg_debug_fold_last_batch")

    def _debug_pick_best(self) -> N.EgUpdateCandidate:
        """Test hook (eg_debug_pick_best): the update's candidate record of the last batch."""
        cand = N.EgUpdateCandidate()
        N.check(N.lib().eg_debug_pick_best(self.h, C.byref(cand)), "eg_debug_pick_best")
        return cand

    def _debug_refine_pick(self, mode: int = 1):
        """Test hook (eg_debug_refine_pick): (step entry, base block [PLAN_BLOCK_BYTES] as the kernel left it) over the last batch."""
        entry = N.EgDebugRefineEntry()
        base = np.zeros(N.PLAN_BLOCK_BYTES, np.uint8)
        N.check(N.lib().eg_debug_refine_pick(self.h, int(mode), C.byref(entry), _p(base, C.c_uint8)), "eg_debug_refine_pick")
        return entry, base

    def _debug_refine_pick_many(self, seg_first, seg_count, mode: int = 1):
        """Test hook (eg_debug_refine_pick_many): (the step entries, one per segment; the base blocks [n_segs, PLAN_BLOCK_BYTES] as the kernel
        left them) over the last batch cut into the given segments."""
        first = np.ascontiguousarray(seg_first, np.uint32); count = np.ascontiguousarray(seg_count, np.uint32)
        assert first.shape == count.shape and first.ndim == 1
        entries = (N.EgDebugRefineEntry * max(len(first), 1))()
        base = np.zeros((max(len(first), 1), N.PLAN_BLOCK_BYTES), np.uint8)
        N.check(N.lib().eg_debug_refine_pick_many(self.h, int(mode), _p(first, C.c_uint32), _p(count, C.c_uint32), len(first), entries, _p(base, C.c_uint8)),
                "eg_debug_refine_pick_many")
        return list(entries), base

    def _debug_repair_pick_many(self, seg_first, seg_count, mode: int = 1, weights=None):
        """Test hook (eg_debug_repair_pick_many): (the repair entries, one per segment; the base blocks [n_segs, PLAN_BLOCK_BYTES] as the
        kernel left them) over the last batch, crafted and judged (_debug_constrain_last_batch), cut into the given segments."""
        first = np.ascontiguousarray(seg_first, np.uint32); count = np.ascontiguousarray(seg_count, np.uint32)
        assert first.shape == count.shape and first.ndim == 1
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        entries = (N.EgDebugRepairEntry * max(len(first), 1))()
        base = np.zeros((max(len(first), 1), N.PLAN_BLOCK_BYTES), np.uint8)
        N.check(N.lib().eg_debug_repair_pick_many(self.h, int(mode), None if w is None else _p(w, C.c_double), _p(first, C.c_uint32), _p(count, C.c_uint32),
                                                  len(first), entries, _p(base, C.c_uint8)), "eg_debug_repair_pick_many")
        return list(entries), base

    def _debug_breed_begin(self, cap: int, mask: int, mode: int = 1) -> None:
        """Test hook (eg_debug_breed_begin): the private archive of eg_breed_plans / eg_explore_plans started empty, canary everywhere."""
        N.check(N.lib().eg_debug_breed_begin(self.h, int(cap), int(mask), int(mode)), "eg_debug_breed_begin")

    def _debug_breed_chunk(self, metrics, status, first_index: int) -> None:
        """Test hook (eg_debug_breed_chunk): a chunk of synthetic records with these metrics [n,4] and status [n] and tagged plan blocks,
        folded into the private archive and gathered."""
        m = np.ascontiguousarray(metrics, dtype=np.float64).reshape(-1, 4)
        st = np.ascontiguousarray(status, dtype=np.int32)
        assert st.shape == (len(m),)
        N.check(N.lib().eg_debug_breed_chunk(self.h, _p(m, C.c_double), _p(st, C.c_int32), len(m), C.c_uint64(int(first_index))), "eg_debug_breed_chunk")

    def _debug_breed_turnover(self, kind: int, next_array: int, m_first: int = 0) -> None:
        """Test hook (eg_debug_breed_turnover): k_breed_turnover (N.DEBUG_TURNOVER_BREED) or k_explore_turnover (N.DEBUG_TURNOVER_EXPLORE)."""
        N.check(N.lib().eg_debug_breed_turnover(self.h, int(kind), int(next_array), C.c_int64(int(m_first))), "eg_debug_breed_turnover")

    def _debug_breed_fetch(self) -> dict:
        """Test hook (eg_debug_breed_fetch): {state, blocks [256, PLAN_BLOCK_BYTES], arrays (the two parent / frontier arrays, likewise),
        readback, counters: uint8 arrays; tags: uint64 [256], n_draws of the record slots}."""
        state = np.zeros(N.DEBUG_PARETO_STATE_BYTES, np.uint8)
        blocks, a0, a1 = (np.zeros((N.PARETO_MAX, N.PLAN_BLOCK_BYTES), np.uint8) for _ in range(3))
        readback = np.zeros(N.DEBUG_BREED_READBACK_BYTES, np.uint8)
        counters = np.zeros(16, np.uint8)
        tags = np.zeros(N.PARETO_MAX, np.uint64)
        N.check(N.lib().eg_debug_breed_fetch(self.h, state.ctypes.data_as(C.c_void_p), _p(blocks, C.c_uint8), _p(a0, C.c_uint8), _p(a1, C.c_uint8), _p(readback, C.c_uint8),
                                             counters.ctypes.data_as(C.c_void_p), _p(tags, C.c_uint64)), "eg_debug_breed_fetch")
        return {"state": state, "blocks": blocks, "arrays": (a0, a1), "readback": readback, "counters": counters, "tags": tags}

    def fetch_scores(self, n_episodes: int) -> np.ndarray:
        s = np.zeros(n_episodes)
        N.check(N.lib().eg_fetch_scores(self.h, _p(s, C.c_double)), "eg_fetch_scores")
        return s

    def fetch_episode_lists(self, episode: int):
        m = np.zeros(4); nr = np.zeros(N.YEARS, np.int32); nd = np.zeros(N.YEARS, np.int32)
        rl = np.zeros(N.RUN_CAP, np.uint8); dl = np.zeros(N.DEF_CAP, np.uint8)
        N.check(N.lib().eg_fetch_episode_lists(self.h, episode, _p(m, C.c_double), _p(nr, C.c_int32), _p(rl, C.c_uint8),
                                               _p(nd, C.c_int32), _p(dl, C.c_uint8)), "eg_fetch_episode_lists")
        return m, nr, rl, nd, dl

    def debug_fill_lds(self, value: int) -> None:
        """Test hook: leave `value` in every LDS word of every CU (LDS is not cleared between workgroups)."""
        N.check(N.lib().eg_debug_fill_lds(self.h, C.c_uint32(value & 0xFFFFFFFF)), "eg_debug_fill_lds")

    def find_suitable_location_xy(self, gen_type: int, generators_xy=(), size_penalty: float = 1.0, year_index: int = 0):
        """MetalLocationSearch::find_suitable_location with the reference's signature (gpu/metal_location_search.rs:96-103):
        further generators at arbitrary coordinates, an f32 size penalty.  Returns ((x, y) or None, best score)."""
        gx = np.ascontiguousarray([p[0] for p in generators_xy], dtype=np.float64)
        gy = np.ascontiguousarray([p[1] for p in generators_xy], dtype=np.float64)
        x, y, score, found = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        N.check(N.lib().eg_find_suitable_location(self.h, year_index, gen_type, _p(gx, C.c_double) if len(gx) else None,
                                                  _p(gy, C.c_double) if len(gy) else None, len(gx), C.c_float(size_penalty),
                                                  C.byref(x), C.byref(y), C.byref(found), C.byref(score)), "eg_find_suitable_location")
        return ((x.value, y.value) if found.value else None), score.value

    def find_suitable_location(self, gen_type: int, year_index: int = 0, extra_cells=()):
        """The same search as the rollout kernels run it (generators on the 1 km grid): returns (cell or -1, best score)."""
        cells = np.ascontiguousarray(list(extra_cells), dtype=np.uint16)
        cell, score = C.c_int32(), C.c_double()
        N.check(N.lib().eg_place(self.h, gen_type, year_index, _p(cells, C.c_uint16) if len(cells) else None, len(cells),
                                 C.byref(cell), C.byref(score)), "eg_place")
        return cell.value, score.value


class _Rank(Engine):
    """A rank's context inside a Group: Engine's per-context queries (fetch, timing, memory report), owned by the group."""

    def __init__(self, handle, world: World):
        self.h = handle
        self.world = world

    def close(self):
        self.h = None      # (eg_group_destroy destroys it)

    __del__ = close


class Group:
    """One eg_group: N ranks (one context each, devices may repeat) driven from this thread; include/eirgrid_hip.h eg_group_*."""

    def __init__(self, world: World, devices=(0, 0)):
        L = N.lib()
        if L.eg_device_count() <= 0:
            raise N.EirgridError("no HIP device visible: eirgrid_amd runs on MI355X (gfx950) only and has no CPU path")
        w, self._keep = _world_struct(world)
        self._devices = np.ascontiguousarray(devices, dtype=np.int32)
        self.h = L.eg_group_create(_p(self._devices, C.c_int32), len(self._devices), C.byref(w))
        if not self.h:
            raise N.EirgridError(L.eg_last_error().decode())
        self.world = world
        self.ranks = [_Rank(L.eg_group_rank(self.h, r), world) for r in range(len(self._devices))]

    @property
    def n_ranks(self) -> int:
        return len(self.ranks)

    def close(self):
        if getattr(self, "h", None):
            for r in getattr(self, "ranks", []):
                r.close()
            try:
                N.lib().eg_group_destroy(self.h)
            except TypeError:      # interpreter shutdown
                pass
            self.h = None

    __del__ = close

    def push(self, weights: ActionWeights, enable_energy_sales=True, write_yearly=True):
        opts = Engine._opts(enable_energy_sales, False, write_yearly)
        N.check(N.lib().eg_group_push(self.h, weights.h, C.byref(opts)), "eg_group_push")

    def step(self, seed: int, first_episode_index: int, n_global: int, replay_period: int, noise_seed: int):
        N.check(N.lib().eg_group_step(self.h, C.c_uint64(seed & (2**64 - 1)), C.c_uint64(first_episode_index), n_global,
                                      replay_period, C.c_uint64(noise_seed & (2**64 - 1))), "eg_group_step")

    def pull(self, rank: int, weights: ActionWeights):
        N.check(N.lib().eg_group_pull(self.h, rank, weights.h), "eg_group_pull")

    def replay_hoist(self, on: bool = True) -> None:
        N.check(N.lib().eg_group_replay_hoist(self.h, int(bool(on))), "eg_group_replay_hoist")

    def track_best_result(self, cost_only: bool = False, on: bool = True) -> None:
        N.check(N.lib().eg_group_best_result_track(self.h, 0 if not on else (2 if cost_only else 1)), "eg_group_best_result_track")

    def fetch_best_result(self):
        """(global index, record) of the run the reference would summarise and export over every rank's results, or (None, None)."""
        res = BatchResult.alloc(1)
        out = res.struct()
        state = C.c_int32(0); index = C.c_int64(-1)
        N.check(N.lib().eg_group_fetch_best_result(self.h, C.byref(out), C.byref(state), C.byref(index)), "eg_group_fetch_best_result")
        return (int(index.value), res) if state.value == 1 else (None, None)

    def track_top_k(self, k: int, cost_only: bool = False) -> None:
        """The top-K archive over every rank's results (eg_group_top_k_track): one context's archive over the same episodes."""
        N.check(N.lib().eg_group_top_k_track(self.h, int(k), 0 if k == 0 else (2 if cost_only else 1)), "eg_group_top_k_track")

    def fetch_top_k(self):
        """(BatchResult of the n_held entries in rank order, their rank scores, their global indices), records from the ranks that ran them."""
        return _fetch_top_k(N.lib().eg_group_fetch_top_k, self.h, "eg_group_fetch_top_k")
