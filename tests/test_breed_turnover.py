"""CPU: the crafted generations of tests/test_gpu_breed_turnover.py and the restatement they are compared with — what k_breed_gather,
k_breed_turnover (csrc/eg_breed.h) and k_explore_turnover (csrc/eg_explore.h) must leave in the private archive of eg_breed_plans /
eg_explore_plans, its block slots, the two parent / frontier arrays and the readback buffer, byte for byte, when they are driven through
the test hooks eg_debug_breed_begin / _chunk / _turnover / _fetch (include/eirgrid_hip.h).  Here: the restatement (Archive: the Front of
tests/test_pareto.py with the slot rule of csrc/eg_pareto.h step 5 and a model of the device's memory), every scenario built by a
function of this file and run on the restatement alone with the properties it was built for asserted — so a scenario that stops doing
what it was built for fails here, not silently on the GPU —, the exported symbols and the refusals that need no device.  No GPU."""
import os
import re
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from tests.test_pareto import Front, front, oriented, valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("eg_debug_breed_begin", "eg_debug_breed_chunk", "eg_debug_breed_turnover", "eg_debug_breed_fetch")
# layout constants (include/eirgrid_hip.h, the debug section)
SLOTS, BLOCK, WORDS = N.PARETO_MAX, N.PLAN_BLOCK_BYTES, N.PLAN_BLOCK_BYTES // 4
HEADER, ROW, OFFSETS = N.DEBUG_BREED_HEADER_BYTES, N.DEBUG_BREED_ROW_BYTES, N.DEBUG_BREED_BLOCK_OFFSETS
CANARY = N.DEBUG_BREED_CANARY
CANARY64 = int.from_bytes(bytes([CANARY]) * 8, "little")
BREED, EXPLORE = N.DEBUG_TURNOVER_BREED, N.DEBUG_TURNOVER_EXPLORE
ENTRY = np.dtype([("metrics", "<f8", 4), ("score", "<f8"), ("index", "<i8"), ("slot", "<i4"), ("pad", "<i4")])
assert ENTRY.itemsize == N.DEBUG_PARETO_ENTRY_BYTES and ROW == 64 + 2 * 4 * 28 and OFFSETS + ROW - 64 <= BLOCK

FAILED = -2              # EG_EP_NO_LOCATION: any status other than EG_EP_OK
FAR = 2**40 + 5          # a first variant number far above 2^32
SIZES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)      # archive sizes around the four ballot words of k_explore_turnover
SUFFIX_STARTS = (0, 1, 63, 64, 65, 128, 192, 255, 256)               # the entry the new suffix starts at (256: nobody is new)
WINDOW_N = (1, 63, 64, 65, 1000)                                     # chunk sizes of the window and counting cases
BIG_N = N.CROSS_MAX_VARIANTS                                         # ... and the one case at a full launch


def tag_block(g):
    """Block of variant number g as eg_debug_breed_chunk writes it: word w = ((g * TAG_MUL mod 2^64) >> 32) + w mod 2^32."""
    h = ((int(g) * N.DEBUG_BREED_TAG_MUL) & (2**64 - 1)) >> 32
    return ((h + np.arange(WORDS, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype("<u4").view(np.uint8)


def score_of(mode):
    from eirgrid_amd.engine import rank_score
    return lambda row: rank_score(np.ascontiguousarray(row), mode == 2)


# ---- the restatement (imports nothing from the feature beyond the layout constants above) ----------------------------------------------

class Archive(Front):
    """tests/test_pareto.py's Front with what the private archive of a generation keeps beside it.
    SLOTS (csrc/eg_pareto.h step 5): a held entry keeps its slot; the new entries, in ascending index, take the lowest free slot below cap.
    BLOCKS: slot s holds the block (and the record, whose tag is the number) of the last entry that owned it — a freed slot keeps it until
    it is retaken — or canary when it was never owned.  n_valid runs over the chunks of a generation.  The device's memory is modelled
    byte for byte from the start (`begin`): the state with its entries (those beyond n_held stay what an earlier fold left there), the
    block slots, the record tags, both parent / frontier arrays and the readback buffer (rows and positions beyond a turnover's count stay
    what they were: canary unless an earlier turnover wrote them)."""

    def __init__(self, cap, mask, score, mode=1):
        super().__init__(cap, mask, score)
        self.mode = mode
        self.slot = np.zeros(0, np.int64)
        self.owner = [None] * SLOTS
        self.n_valid = 0
        self.top = -1                      # the highest variant number seen: numbers only grow
        self.entries = np.zeros(SLOTS, ENTRY)
        self.blocks = np.full((SLOTS, BLOCK), CANARY, np.uint8)
        self.tags = np.full(SLOTS, CANARY64, np.uint64)
        self.arrays = [np.full((SLOTS, BLOCK), CANARY, np.uint8) for _ in range(2)]
        self.readback = np.full(HEADER + SLOTS * ROW, CANARY, np.uint8)
        self.last = {}                     # what the last fold did (the scenarios' preconditions)

    def fold(self, metrics, status, first):
        """Front.fold, then the slots and the gather.  Rows with the same oriented coordinates are reduced to the one of lowest (index,
        position) before the O(n^2) pass — exactly the row that beats the others — so a chunk of 16 384 records over a few hundred distinct
        points stays cheap; Run.chunk holds the result against Front.fold for every chunk of at most 4 096 records."""
        metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 4)
        n = len(metrics)
        assert first > self.top, "variant numbers only grow"
        self.top = first + n - 1
        ok = valid(metrics, status)
        self.n_valid += int(ok.sum())
        was = dict(zip(self.index.tolist(), self.slot.tolist()))
        m = np.concatenate([self.m, metrics[ok]])
        idx = np.concatenate([self.index, first + np.nonzero(ok)[0].astype(np.int64)])
        v = oriented(m, self.mask) + 0.0      # (-0.0 + 0.0 = +0.0: one point)
        order = np.lexsort((np.arange(len(v)), idx))
        _, firsts = np.unique(v[order], axis=0, return_index=True) if len(v) else (None, np.zeros(0, np.int64))
        cand = np.sort(order[firsts])
        alive = cand[front(m[cand], idx[cand], self.mask)]
        keep, cut = alive, alive[:0]
        if len(alive) > self.cap:
            s = np.array([self.score(m[p]) for p in alive])
            key = np.where(np.isnan(s), -np.inf, s)
            by = np.array(sorted(range(len(alive)), key=lambda r: (-key[r], idx[alive[r]], alive[r])))
            self.n_dropped += len(alive) - self.cap
            keep, cut = alive[by[:self.cap]], alive[by[self.cap:]]
        keep = keep[np.lexsort((keep, idx[keep]))]
        self.m, self.index = m[keep], idx[keep]
        # the slots: held entries keep theirs, new ones take the lowest free below cap
        used = {was[i] for i in self.index.tolist() if i in was}
        freed = set(was.values()) - used
        free = iter(s for s in range(self.cap) if s not in used)
        slot, new, retaken = [], [], 0
        for i in self.index.tolist():
            if i in was:
                slot.append(was[i])
                continue
            s = next(free)
            slot.append(s); new.append(i)
            retaken += s in freed
            self.owner[s] = i; self.blocks[s] = tag_block(i); self.tags[s] = i      # the gather, and the record k_pareto_finalize copies
        self.slot = np.array(slot, np.int64)
        assert len(set(slot)) == len(slot) and all(self.owner[s] == i for s, i in zip(slot, self.index.tolist()))
        e = self.entries[:len(keep)]
        e["metrics"], e["score"], e["index"], e["slot"], e["pad"] = self.m, self.scores(), self.index, self.slot, 0
        self.last = {"n": n, "first": first, "alive": len(alive), "new": new, "retaken": retaken, "cut": sorted(idx[cut].tolist()),
                     "left": sorted(set(was) - set(self.index.tolist())), "moved": int((self.slot != np.arange(len(slot))).sum())}
        return self

    def turnover(self, kind, nxt, m_first=0):
        """k_breed_turnover: entry r to position r and row r.  k_explore_turnover: the entries with index >= m_first, at their count among
        those.  Returns the number of rows written."""
        n = len(self.index)
        rows, n_new = np.arange(n), 0
        if kind == EXPLORE:
            new = self.index >= m_first
            n_new = int(new.sum())
            assert new[n - n_new:].all() and not new[:n - n_new].any(), "entries stand in ascending index: the new ones are a suffix"
            rows = np.arange(n - n_new, n)
        for pos, r in enumerate(rows):
            blk = self.blocks[self.slot[r]]
            self.arrays[nxt][pos] = blk
            at = HEADER + pos * ROW
            self.readback[at:at + ROW] = np.frombuffer(self.entries[r].tobytes() + bytes(8) + blk[OFFSETS:OFFSETS + ROW - 64].tobytes(), np.uint8)
        self.readback[:HEADER] = np.frombuffer(struct.pack("<iiqqq", n, n_new, self.n_dropped, self.n_valid, 0), np.uint8)
        self.n_valid = 0
        if kind == BREED:      # the archive of a generation of crosses starts the next one empty
            self.m, self.index, self.slot, self.n_dropped = np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, np.int64), 0
        return len(rows)

    def state(self):
        return np.frombuffer(struct.pack("<iiiiqq", self.cap, len(self.index), self.mask, self.mode, self.n_dropped, 0) + self.entries.tobytes(), np.uint8)

    def counters(self):
        return np.frombuffer(struct.pack("<QII", self.n_valid, 0, 0), np.uint8)


class Run:
    """A scenario's steps on the restatement and — with an engine — on the device, `check(engine, archive, what)` after every step."""

    def __init__(self, eng=None, check=None, shadow=True):
        self.eng, self.check, self.shadow_on = eng, check, shadow
        self.arch = self.shadow = None
        self.steps = 0

    def _after(self, what):
        self.steps += 1
        if self.eng is not None:
            self.check(self.eng, self.arch, (self.steps, what))

    def begin(self, cap, mask, mode=1):
        self.arch = Archive(cap, mask, score_of(mode), mode)
        self.shadow = Front(cap, mask, score_of(mode))
        if self.eng is not None:
            self.eng._debug_breed_begin(cap, mask, mode)
        self._after("begin")

    def chunk(self, m, st, first):
        m = np.ascontiguousarray(m, dtype=np.float64); st = np.ascontiguousarray(st, dtype=np.int32)
        self.arch.fold(m, st, first)
        if self.shadow_on and len(m) <= 4096:      # the restatement's short cut against the plain Front
            self.shadow.fold(m, st, first)
            assert self.shadow.index.tolist() == self.arch.index.tolist() and self.shadow.m.tobytes() == self.arch.m.tobytes()
            assert self.shadow.n_dropped == self.arch.n_dropped
        else:
            self.shadow.m, self.shadow.index, self.shadow.n_dropped = self.arch.m, self.arch.index, self.arch.n_dropped
        if self.eng is not None:
            self.eng._debug_breed_chunk(m, st, first)
        self._after(("chunk", len(m), first))
        return self.arch.last

    def turnover(self, kind, nxt, m_first=0):
        rows = self.arch.turnover(kind, nxt, m_first)
        if kind == BREED:
            self.shadow.m, self.shadow.index, self.shadow.n_dropped = self.arch.m, self.arch.index, 0
        if self.eng is not None:
            self.eng._debug_breed_turnover(kind, nxt, m_first)
        self._after(("turnover", kind, nxt, m_first))
        return rows

    def header(self):
        return struct.unpack("<iiqqq", self.arch.readback[:HEADER].tobytes())


# ---- points: small integers, as tests/test_gpu_pareto.py's --------------------------------------------------------------------------------

def ok(n):
    return np.zeros(n, np.int32)


def anti(ks):
    """Mutually non-dominated points under masks 5 and 15: emissions 2000 + 4k against cost 20000 - 4k; opinion and reliability small and
    mixed.  The rank score falls with k (emissions above net zero), so a truncation keeps the lowest k."""
    k = np.asarray(list(ks), dtype=np.float64)
    return np.stack([2000.0 + 4.0 * k, np.mod(k, 3.0), 20000.0 - 4.0 * k, np.mod(k, 2.0)], axis=1)


def below(p):
    """Points the points p dominate under both masks (one worse in emissions and cost)."""
    q = np.array(p, dtype=np.float64)
    q[:, 0] += 1.0; q[:, 2] += 1.0
    return q


def above(p):
    """Points that dominate the points p, and no other point of an anti() set, under both masks."""
    q = np.array(p, dtype=np.float64)
    q[:, 0] -= 1.0; q[:, 2] -= 1.0; q[:, 1] = 9.0; q[:, 3] = 9.0
    return q


def mixed(rng, *parts):
    m = np.concatenate(parts)
    return m[rng.permutation(len(m))]


def numbers_are_distinct(numbers):
    """The tags of the variant numbers a scenario uses tell them apart: no two blocks share a word."""
    h = np.sort(np.array([((int(g) * N.DEBUG_BREED_TAG_MUL) & (2**64 - 1)) >> 32 for g in numbers], np.int64))
    return len(h) < 2 or int(np.diff(h).min()) >= WORDS


# ---- the scenarios (each asserts what it was built for, from the restatement alone) ------------------------------------------------------

def case1_breed(R, mask):
    """A generation per size: two chunks (every point of the antichain beside one it dominates, shuffled), then k_breed_turnover into the
    arrays 0 and 1 alternately."""
    rng = np.random.default_rng(10 + mask)
    first = 2**32 - 700      # (the numbers cross 2^32 on the way)
    for g, size in enumerate(SIZES):
        R.begin(256, mask)
        for a, b in ((0, size // 2), (size // 2, size)):
            if b > a:
                p = anti(range(a, b))
                R.chunk(mixed(rng, p, below(p)), ok(2 * (b - a)), first)
                first += 2 * (b - a) + 3
        assert len(R.arch.index) == size and R.arch.n_dropped == 0
        assert size < 3 or (R.arch.index != R.arch.index[0] + np.arange(size)).any()      # an entry's index is not its position
        assert R.turnover(BREED, g % 2) == size
        assert R.header() == (size, 0, 0, 2 * size, 0) and len(R.arch.index) == 0
    assert first > 2**32


def case1_explore(R, mask):
    """One archive grown to every size in turn, the members that entered turned over after each chunk; then, at 256 entries, the new
    suffix started at every entry of SUFFIX_STARTS, at an m_first between two indices, and at 0."""
    rng = np.random.default_rng(20 + mask)
    R.begin(256, mask)
    first, held = 5, 0
    for g, size in enumerate(SIZES):
        p = anti(range(held, size))
        R.chunk(mixed(rng, p, below(p)), ok(2 * len(p)), first)
        assert len(R.arch.index) == size
        assert R.turnover(EXPLORE, g % 2, first) == size - held and R.header() == (size, size - held, 0, 2 * len(p), 0)
        first += 2 * len(p) + 3
        held = size
    idx = R.arch.index.tolist()
    assert len(idx) == 256 and numbers_are_distinct(idx)
    for g, k in enumerate(SUFFIX_STARTS):
        assert R.turnover(EXPLORE, g % 2, idx[k] if k < 256 else idx[-1] + 1) == 256 - k and R.header() == (256, 256 - k, 0, 0, 0)
    gap = next(k for k in range(100, 256) if idx[k] - idx[k - 1] > 1)
    assert R.turnover(EXPLORE, 1, idx[gap] - 1) == 256 - gap
    assert R.turnover(EXPLORE, 0, 0) == 256


def case_evict(R, mask, kind, cap=256, n0=200, n_new=25):
    """Cases 2 and 3.  An antichain of n0 (cap of them stay); two chunks that each dominate every third held entry and add n_new points
    of better rank score; then points equal to held ones at higher numbers.  kind EXPLORE: a turnover behind every chunk; BREED: one at
    the end.  Returns what the chunks did."""
    rng = np.random.default_rng(30 + mask + cap)
    R.begin(cap, mask)
    first, did = 11, []

    def chunk(m):
        nonlocal first
        did.append(R.chunk(m, ok(len(m)), first))
        if kind == EXPLORE:
            R.turnover(EXPLORE, len(did) % 2, first)
            assert R.header()[1] == len(did[-1]["new"]) and R.header()[3] == len(m)
        first += len(m) + 2

    chunk(mixed(rng, anti(range(n0))))
    for rnd in (1, 2):
        before = set(R.arch.index.tolist())
        chunk(mixed(rng, above(R.arch.m[::3]), anti(range(-rnd * n_new, -(rnd - 1) * n_new))))
        assert len(before - set(R.arch.index.tolist())) >= len(before) // 3      # at least the dominated third left
    held, blocks, state = R.arch.index.tolist(), R.arch.blocks.copy(), R.arch.state().copy()
    equal = R.arch.m[::5].copy()
    chunk(equal)
    assert did[-1]["new"] == [] and R.arch.index.tolist() == held and R.arch.blocks.tobytes() == blocks.tobytes() and R.arch.state().tobytes() == state.tobytes()
    if kind == BREED:
        R.turnover(BREED, 1)
        assert R.header() == (len(held), 0, sum(len(d["cut"]) for d in did), sum(d["n"] for d in did), 0)
    assert numbers_are_distinct(o for o in R.arch.owner if o is not None)
    return did


def case_window(R, mask, kind, n):
    """Case 4.  A chunk of 70 that ends at FAR - 1, then a chunk of n at FAR whose records 0 and n - 1 enter the archive (pool blocks 0
    and n - 1) while entries of the chunk before stay, then a chunk of 9 behind it; a turnover.  Everything else in the middle chunk is a
    point that a point of the chunk dominates, or equals."""
    rng = np.random.default_rng(40 + mask + n)
    R.begin(256, mask)
    p = anti(range(100, 170))
    R.chunk(p[rng.permutation(70)], ok(70), FAR - 70)
    assert FAR - 1 in R.arch.index.tolist()
    k = min(n, 40)                                            # points of the chunk that enter: some beside the held ones, some above them
    enter = np.concatenate([anti(range(170, 170 + (k + 1) // 2)), above(anti(range(100, 100 + 2 * (k // 2), 2)))])[:k]
    enter = enter[rng.permutation(k)]
    m = below(enter)[rng.integers(0, k, n)]
    at = list(dict.fromkeys([0, n - 1] + (1 + rng.permutation(max(n - 2, 0))).tolist()))[:k]      # k distinct places, 0 and n - 1 among them
    m[at] = enter
    did = R.chunk(m, ok(n), FAR)
    idx = R.arch.index.tolist()
    assert FAR in idx and FAR + n - 1 in idx and len(did["new"]) == k
    assert sum(i < FAR for i in idx) >= 30 and (n < 4 or len(did["left"]) >= 1)      # held from the chunk before; and some of them left
    R.chunk(mixed(rng, anti(range(300, 305)), above(anti(range(101, 109, 2)))), ok(9), FAR + n)
    assert FAR + n - 1 in R.arch.index.tolist() or n < 4
    R.turnover(kind, 1, FAR)
    assert numbers_are_distinct(o for o in R.arch.owner if o is not None)
    return did


def bad_records(rng, m, st):
    """Failed statuses and NaN metrics sprinkled in, at records 0 and n - 1 too (n >= 4); -0.0 and infinities, which are valid."""
    n = len(m)
    if n >= 4:
        st[0] = FAILED; m[n - 1, 2] = np.nan
        st[rng.uniform(size=n) < 0.1] = FAILED
        m[rng.uniform(size=n) < 0.1, rng.integers(0, 4)] = np.nan
        m[1] = (-0.0, 1.0, 30000.0, 1.0)          # the lowest emissions: on the front
        m[2] = (50.0, 0.0, np.inf, 0.0)           # valid, dominated by record 1
        if n >= 6:
            m[n - 2] = (0.0, 1.0, 30000.0, 1.0)   # +0.0: record 1 again, later
            m[n - 3] = (-np.inf, 0.0, 40000.0, 0.0)
    return m, st


def case_count(R, mask, kind, n):
    """Case 5.  Two generations without a `begin` between them, each of a chunk of n and a chunk of 37 with invalid records sprinkled in."""
    rng = np.random.default_rng(50 + mask + n)
    R.begin(256, mask)
    first, sums = 3, []
    for g in range(2):
        gen_first, total = first, 0
        for size in (n, 37):
            p = anti(rng.integers(g * 50, g * 50 + 120, size))
            m, st = bad_records(rng, mixed(rng, p), ok(size))
            want = int(valid(m, st).sum())
            assert size < 4 or 0 < want < size
            R.chunk(m, st, first)
            total += want
            first += size
            assert R.arch.n_valid == total
        R.turnover(kind, g % 2, gen_first)
        assert R.header()[3] == total and R.arch.n_valid == 0
        sums.append(total)
    assert min(sums) > 0      # (a count carried over from the first generation would show in the second header)
    return sums


def case_empty(R, mask, kind):
    """A generation without a valid variant: nothing is held, nothing is written but the header."""
    R.begin(256, mask)
    m = anti(range(50))
    m[::2, 0] = np.nan
    st = ok(50); st[1::2] = FAILED
    R.chunk(m, st, 9)
    assert R.turnover(kind, 0, 9) == 0 and R.header() == (0, 0, 0, 0, 0)
    canary = bytes([CANARY])
    assert all(a.tobytes() == canary * a.size for a in R.arch.arrays) and R.arch.readback[HEADER:].tobytes() == canary * (SLOTS * ROW)


# ---- CPU tests -----------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_hooks(built):
    L = N.lib()
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    for name in HOOKS:
        assert hasattr(L, name) and name in N.EXPORTS, name
        assert re.search(rf"\bint32_t {name}\(", header), name
    for name, value in (("CANARY", CANARY), ("ROW_BYTES", ROW), ("HEADER_BYTES", HEADER), ("BLOCK_OFFSETS", OFFSETS)):
        assert int(re.search(rf"#define EG_DEBUG_BREED_{name} (\w+)", header).group(1), 0) == value, name
    assert int(re.search(r"#define EG_DEBUG_BREED_TAG_MUL (\w+?)ull", header).group(1), 0) == N.DEBUG_BREED_TAG_MUL
    assert (BREED, EXPLORE) == (int(re.search(r"#define EG_DEBUG_TURNOVER_BREED (\d+)", header).group(1)), int(re.search(r"#define EG_DEBUG_TURNOVER_EXPLORE (\d+)", header).group(1)))
    assert N.DEBUG_PARETO_STATE_BYTES == 32 + 256 * 56 and N.DEBUG_BREED_READBACK_BYTES == 32 + 256 * 288 and N.CROSS_MAX_VARIANTS == 16384


def test_hooks_refuse_a_null_context_before_any_device(built):
    L = N.lib()
    for name, args in (("eg_debug_breed_begin", (None, 8, 15, 1)), ("eg_debug_breed_chunk", (None, None, None, 1, 0)),
                       ("eg_debug_breed_turnover", (None, BREED, 0, 0)), ("eg_debug_breed_fetch", (None,) * 8)):
        assert getattr(L, name)(*args) == N.EG_ERR_BAD_ARG, name
        assert L.eg_last_error().decode() == name + ": bad argument"


def test_tags_tell_numbers_and_words_apart():
    a, b = tag_block(FAR).view("<u4"), tag_block(FAR + 1).view("<u4")
    assert len(a) == WORDS == 2208 and (np.diff(a.astype(np.int64)) % 2**32 == 1).all()
    assert int(a[0]) == ((FAR * 0x9E3779B97F4A7C15) % 2**64) >> 32 and a[0] != tag_block(5)[:4].view("<u4")[0]      # the high half counts
    assert not set(a.tolist()) & set(b.tolist())
    assert numbers_are_distinct(range(FAR - 70, FAR + BIG_N + 9)) and numbers_are_distinct(range(2**32 - 700, 2**32 + 3000))
    assert not numbers_are_distinct([7, 7])
    assert int(tag_block(3)[OFFSETS:OFFSETS + 4].view("<u4")[0]) == (int(tag_block(3)[:4].view("<u4")[0]) + OFFSETS // 4) % 2**32


def test_archive_slot_rule_by_hand(built):
    """cap 4 under mask 5.  Numbers 10..12: an antichain in slots 0, 1, 2.  Number 20 dominates 11: slot 1 is freed and retaken in the
    same fold by 20, and 21 — beside them — takes slot 3.  Number 30 dominates 12 and 21 (slots 2 and 3 freed, 2 retaken); slot 3 keeps
    21's block."""
    a = Archive(4, 5, score_of(1))
    p = anti([0, 1, 2])
    a.fold(p, ok(3), 10)
    assert a.slot.tolist() == [0, 1, 2] and a.owner == [10, 11, 12] + [None] * 253
    a.fold(np.concatenate([above(p[1:2]), anti([3])]), ok(2), 20)
    assert a.index.tolist() == [10, 12, 20, 21] and a.slot.tolist() == [0, 2, 1, 3] and a.last["retaken"] == 1 and a.last["moved"] == 2
    both = np.array([[2008.0, 0.0, 19988.0, 0.0]])      # p[2]'s emissions and number 21's cost
    a.fold(both, ok(1), 30)
    assert a.index.tolist() == [10, 20, 30] and a.slot.tolist() == [0, 1, 2] and a.owner[:4] == [10, 20, 30, 21] and a.last["left"] == [12, 21]
    assert a.blocks[3].tobytes() == tag_block(21).tobytes() and a.tags[:4].tolist() == [10, 20, 30, 21] and a.tags[4] == CANARY64
    assert a.blocks[4:].tobytes() == bytes([CANARY]) * (252 * BLOCK)
    # explore: the members from number 20 on, at positions 0 and 1 of array 1; the state stays
    state = a.state().tobytes()
    assert a.turnover(EXPLORE, 1, 20) == 2 and a.state().tobytes() == state
    assert a.arrays[1][0].tobytes() == tag_block(20).tobytes() and a.arrays[1][1].tobytes() == tag_block(30).tobytes()
    assert a.arrays[1][2:].tobytes() == bytes([CANARY]) * (254 * BLOCK) and a.arrays[0].tobytes() == bytes([CANARY]) * (256 * BLOCK)
    assert struct.unpack("<iiqqq", a.readback[:HEADER].tobytes()) == (3, 2, 0, 6, 0) and a.n_valid == 0
    row = a.readback[HEADER + ROW:HEADER + 2 * ROW]
    e = np.frombuffer(row[:56].tobytes(), ENTRY)[0]
    assert e["index"] == 30 and e["slot"] == 2 and e["metrics"].tolist() == both[0].tolist() and e["score"] == score_of(1)(both[0])
    assert row[56:64].tolist() == [0] * 8 and row[64:].tobytes() == tag_block(30)[OFFSETS:OFFSETS + 224].tobytes()
    assert a.readback[HEADER + 2 * ROW:].tobytes() == bytes([CANARY]) * (254 * ROW)
    with pytest.raises(AssertionError):
        a.fold(both, ok(1), 30)      # a number that does not grow
    # breed: all three, and the archive is empty afterwards while the slots keep their blocks
    assert a.turnover(BREED, 0) == 3 and len(a.index) == 0 and a.n_dropped == 0 and a.owner[:4] == [10, 20, 30, 21]
    assert struct.unpack("<iiiiqq", a.state()[:32].tobytes()) == (4, 0, 5, 1, 0, 0)
    assert [a.arrays[0][r].tobytes() == tag_block(g).tobytes() for r, g in enumerate((10, 20, 30))] == [True] * 3


@pytest.mark.parametrize("mask", [5, 15])
def test_case1_sizes_across_the_ballot_words(built, mask):
    case1_breed(Run(), mask)
    case1_explore(Run(), mask)


@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
def test_case2_eviction_and_slot_reuse(built, mask, kind):
    R = Run()
    did = case_evict(R, mask, kind)
    assert [len(d["new"]) for d in did[:3]] == [200, 67 + 25, 75 + 25] and all(d["cut"] == [] for d in did)
    for d in did[1:3]:
        assert d["retaken"] >= 10 and d["moved"] >= 40, d      # freed slots retaken within the fold that freed them; slot != position
    assert did[1]["retaken"] == 67 and len(did[1]["left"]) == 67
    owners = [o for o in R.arch.owner if o is not None]
    assert did[3]["n"] == len(range(0, 250, 5)) and did[3]["first"] > max(owners)      # the equal points arrive at higher numbers
    assert len(owners) == 250 and R.arch.owner[250:] == [None] * 6


@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
@pytest.mark.parametrize("cap,n_new", [(8, 5), (256, 150)])
def test_case3_capacity(built, mask, kind, cap, n_new):
    R = Run()
    did = case_evict(R, mask, kind, cap=cap, n_new=n_new)
    assert len(did[0]["cut"]) == max(0, 200 - cap)
    for d in did[1:3]:
        assert d["alive"] > cap and len(d["cut"]) == d["alive"] - cap
        assert any(d["first"] <= g < d["first"] + d["n"] for g in d["cut"])      # a point of the chunk was dropped: no block was gathered for it
        assert any(g < d["first"] for g in d["cut"])                              # ... and a held entry lost its place to the truncation
        assert not set(d["cut"]) & set(d["new"]) and len(d["new"]) >= 3
    assert R.arch.n_dropped > 0 or kind == BREED
    owners = [o for o in R.arch.owner if o is not None]
    assert not set(owners) & {g for d in did for g in d["cut"] if g >= d["first"]}      # never in a slot: dropped when it arrived
    if cap == 8:
        assert R.arch.owner[8:] == [None] * 248 and len(owners) == 8


@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
@pytest.mark.parametrize("n", WINDOW_N + (BIG_N,))
def test_case4_the_gathers_window(built, mask, kind, n):
    did = case_window(Run(), mask, kind, n)
    assert FAR in did["new"] and FAR + n - 1 in did["new"] and did["first"] == FAR > 2**40


@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
@pytest.mark.parametrize("n", WINDOW_N + (BIG_N,))
def test_case5_counting(built, mask, kind, n):
    sums = case_count(Run(), mask, kind, n)
    assert all(0 < s <= n + 37 for s in sums)
    case_empty(Run(), mask, kind)
