"""GPU: the lazy penalty field's catch-up of a pair of tiles (csrc/eg_field.h tiles_refresh), one wave per case through the hook
eg_debug_tiles_refresh: a crafted generator list, a radius class, two tiles (the second may be none), the tiles' counters and stored
values in a class field laid out as a slot of the pool holds it.

Expected: a NumPy restatement — for every cell of a tile the class's d/R entries (HostTables "dr", [class][|di|][|dj|], 1.0 from the
radius on) of the generators the tile does not hold yet, multiplied in list order in float64, from the stored value or, for a tile
that holds none, from 1.0.  Compared bit for bit; every other double of the field, the counters of the other tiles included, must
come back as it went in (a lane off the grid stores nothing), the two tiles' counters are the list's length, and the count of
generators folded is the count of pending generators inside either tile's box.

The shapes are the smallest at which the staged fold can go wrong: near sets that end on either side of a pair, of a group of four
and at a full row of 64; generators that reach one tile, the other, both; counters that differ, that are zero over garbage, that
equal the list's length; distances of zero, just below, at and beyond the radius; edge tiles and a round's lone tile; lists that end
and pending ranges that start on and off a block of 64, and a list that goes on beyond the on-chip window."""
import ctypes as C

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import HostTables

pytestmark = pytest.mark.gpu

GRID, TILES, TILE_W, COLS = N.GRID, 49, 8, 7
FIELD_DOUBLES, TILE_COUNTERS = 2624, 2602      # EG_DEBUG_FIELD_DOUBLES, EG_DEBUG_TILE_COUNTERS
SENTINEL = 0.8125                               # what every cell outside the two tiles holds
BATTERY, GAS_CC, NUCLEAR = 12, 7, 5             # generator types of the 3 km, 8 km and 12 km classes (eirgrid_amd/world.py)


@pytest.fixture(scope="module")
def tables(world):
    h = HostTables(world)
    return {"dr": h.f64("dr").reshape(6, 13, 13), "rclass": h.i32("rclass"), "reach": h.i32("reach")}


def _tile_cells(t):
    """(lane's row, lane's column, on the grid) of tile t, a cell per lane"""
    lane = np.arange(64)
    i, j = (t // COLS) * TILE_W + (lane >> 3), (t % COLS) * TILE_W + (lane & 7)
    return i, j, (i < GRID) & (j < GRID)


def _in_box(t, cells, reach):
    gi, gj = cells // GRID, cells % GRID
    r0, c0 = (t // COLS) * TILE_W, (t % COLS) * TILE_W
    return (gi >= r0 - reach) & (gi <= r0 + TILE_W - 1 + reach) & (gj >= c0 - reach) & (gj <= c0 + TILE_W - 1 + reach)


def _expected(dr, rc, t, cells, applied, stored):
    i, j, _ = _tile_cells(t)
    v = np.ones(64) if applied == 0 else stored.copy()
    for g in cells[applied:]:
        di, dj = np.abs(i - int(g) // GRID), np.abs(j - int(g) % GRID)
        f = np.where((di <= 12) & (dj <= 12), dr[rc, np.minimum(di, 12), np.minimum(dj, 12)], 1.0)
        v = v * f      # (list order, float64, one rounding per generator: what the device does, leaving out only factors of exactly 1.0)
    return v


def _run(engine, tables, gen_type, cells, ta, tb, applied_a, applied_b, what, garbage=None):
    """one call of the hook, checked against the restatement; returns the count of generators folded"""
    rc, cells = int(tables["rclass"][gen_type]), np.asarray(cells, np.uint16)
    reach, n = int(tables["reach"][rc]), len(cells)
    rng = np.random.default_rng(ta * 64 + (tb & 63) + n)
    field = np.full(FIELD_DOUBLES, SENTINEL)
    counters = field[TILE_COUNTERS:].view(np.uint16)
    counters[:TILES] = (np.arange(TILES) * 37 + 5) % (n + 1)      # the other tiles': whatever
    stored = {}
    for t, a in ((ta, applied_a), (tb, applied_b)):
        if t < 0:
            continue
        i, j, on = _tile_cells(t)
        stored[t] = rng.uniform(0.01, 1.0, 64) if garbage is None else np.full(64, garbage)
        field[(i * GRID + j)[on]] = stored[t][on]
        counters[t] = a
    before = field.copy()
    folded = C.c_int32(-7)
    N.check(N.lib().eg_debug_tiles_refresh(engine.h, cells.ctypes.data_as(C.POINTER(C.c_uint16)), n, rc, ta, tb,
                                            field.ctypes.data_as(C.POINTER(C.c_double)), C.byref(folded)), "eg_debug_tiles_refresh")
    want = before.copy()
    pending = np.zeros(n, bool)
    for t, a in ((ta, applied_a), (tb, applied_b)):
        if t < 0:
            continue
        i, j, on = _tile_cells(t)
        want[(i * GRID + j)[on]] = _expected(tables["dr"], rc, t, cells.astype(np.int64), a, stored[t])[on]
        want[TILE_COUNTERS:].view(np.uint16)[t] = n
        pending |= (np.arange(n) >= a) & _in_box(t, cells.astype(np.int64), reach)
    diff = np.flatnonzero(field.view(np.uint64) != want.view(np.uint64))
    assert diff.size == 0, (what, diff[:8].tolist(), field[diff[:8]].tolist(), want[diff[:8]].tolist())
    assert folded.value == int(pending.sum()), (what, folded.value, int(pending.sum()))
    return folded.value


def _cell(i, j):
    return i * GRID + j


def _near(rng, t, reach, k, inside_tile=False):
    """k distinct cells inside tile t's box (by default not inside the tile itself: no factor of zero)"""
    r0, c0 = (t // COLS) * TILE_W, (t % COLS) * TILE_W
    box = [(i, j) for i in range(max(r0 - reach, 0), min(r0 + TILE_W + reach, GRID)) for j in range(max(c0 - reach, 0), min(c0 + TILE_W + reach, GRID))
           if inside_tile or not (r0 <= i < r0 + TILE_W and c0 <= j < c0 + TILE_W)]
    return [_cell(*box[p]) for p in rng.permutation(len(box))[:k]]


# tiles far apart: 0 (rows 0-7, columns 0-7) and 32 (rows 32-39, columns 32-39) share no generator of the 8 km class (reach 7)
FAR_A, FAR_B = 0, 32


@pytest.mark.parametrize("ka,kb", [(0, 0), (1, 0), (0, 1), (3, 1), (4, 4), (5, 3), (8, 9), (9, 8), (64, 5), (2, 64)])
def test_near_set_sizes(engine, tables, ka, kb):
    """ka generators near tile a only and kb near tile b only, shuffled into one block of the list with generators near neither: the
    ends of the pairs and of the groups of four, an empty row beside a full one, and rows of unequal length"""
    rng = np.random.default_rng(100 + 65 * ka + kb)
    reach = int(tables["reach"][tables["rclass"][GAS_CC]])
    near_a, near_b = _near(rng, FAR_A, reach, ka), _near(rng, FAR_B, reach, kb)
    neither = _cell(20, 2)      # (row 20: beyond tile 0's box, column 2: beyond tile 32's)
    if max(ka, kb) == 64:       # the full row: the 64 are one block of the list, the rest follows
        cells = (near_a if ka == 64 else near_b) + [int(c) for c in rng.permutation((near_b if ka == 64 else near_a) + [neither] * 20)]
    else:
        cells = [int(c) for c in rng.permutation(near_a + near_b + [neither] * (70 - ka - kb))]
    assert _run(engine, tables, GAS_CC, cells, FAR_A, FAR_B, 0, 0, (ka, kb)) == ka + kb


def test_a_full_row_for_both_tiles(engine, tables):
    """a hundred generators that both of two adjacent tiles need (12 km class): a full row for each from the first block, then a second block"""
    rng = np.random.default_rng(7)
    cells = [_cell(int(i), int(j)) for i, j in zip(rng.integers(16, 24, 100), rng.integers(21, 27, 100))]      # rows 16-23, columns 21-26: the seam of the two tiles
    assert _run(engine, tables, NUCLEAR, cells, 2 * COLS + 2, 2 * COLS + 3, 0, 0, "full rows") == 100


def test_tile_overlap_and_counters(engine, tables):
    """adjacent tiles 16 (rows 16-23, columns 16-23) and 17 (columns 24-31), 3 km class (reach 2): generators that reach a only, b only,
    both, neither; the two counters differ, one is zero over garbage, both equal the list's length"""
    a_only, b_only, both, neither = _cell(18, 15), _cell(20, 33), _cell(19, 23), _cell(40, 40)
    cells = [a_only, both, neither, b_only, both, a_only, b_only, b_only, neither, both, a_only]
    n = len(cells)
    ta, tb = 2 * COLS + 2, 2 * COLS + 3
    for applied_a, applied_b in ((0, 0), (3, 7), (7, 3), (n, 2), (2, n), (n - 1, n - 1)):
        _run(engine, tables, BATTERY, cells, ta, tb, applied_a, applied_b, ("overlap", applied_a, applied_b))
    assert _run(engine, tables, BATTERY, cells, ta, tb, n, n, "nothing to do") == 0
    # a tile that holds none: its values are products from 1.0 whatever is stored (NaN would stick to every product)
    _run(engine, tables, BATTERY, cells, ta, tb, 0, 4, "garbage under a zero counter", garbage=float("nan"))
    _run(engine, tables, BATTERY, cells, ta, tb, 5, 0, "garbage under a zero counter", garbage=float("nan"))
    assert _run(engine, tables, BATTERY, [], ta, tb, 0, 0, "an empty list", garbage=float("nan")) == 0


@pytest.mark.parametrize("gen_type", [BATTERY, GAS_CC, NUCLEAR])
def test_distances(engine, tables, gen_type):
    """generators at distance zero of a cell of the tile, at the last whole distances below the class's radius, exactly at it and beyond"""
    rc = int(tables["rclass"][gen_type])
    reach = int(tables["reach"][rc])
    dr = tables["dr"][rc]
    assert dr[reach, 0] < 1.0 and dr[reach + 1, 0] == 1.0 and dr[0, 0] == 0.0      # (reach + 1 km is the radius itself: d / R = 1 is not below it)
    i0, j0 = 24, 24      # the first cell of tile 24 (rows 24-31, columns 24-31)
    offsets = [(0, 0), (3, 4), (-reach, 0), (0, -reach), (-(reach + 1), 0), (0, -(reach + 1)), (-(reach + 2), 0), (7 + reach, 7), (7 + reach + 1, 7), (7, 7 + reach + 1)]
    offsets += [(-a, -b) for a in range(1, reach + 2) for b in range(1, reach + 2) if reach * reach <= a * a + b * b <= (reach + 1) ** 2 + 1]
    for k, (di, dj) in enumerate(offsets):      # one at a time, then all of them
        _run(engine, tables, gen_type, [_cell(i0 + di, j0 + dj)], 24, -1, 0, 0, ("distance", gen_type, di, dj))
    _run(engine, tables, gen_type, [_cell(i0 + di, j0 + dj) for di, dj in offsets[1:]], 24, 25, 0, 0, ("distances", gen_type))


def test_edge_tiles_and_a_lone_tile(engine, tables):
    """tiles 6 and 48 (three columns wide; 48 three rows as well): the lanes off the grid store nothing; and a lone tile"""
    rng = np.random.default_rng(3)
    reach = int(tables["reach"][tables["rclass"][GAS_CC]])
    cells = _near(rng, 6, reach, 9, inside_tile=True) + _near(rng, 48, reach, 7, inside_tile=True) + _near(rng, 42, reach, 5, inside_tile=True)
    cells = list(rng.permutation(cells))
    for ta, tb in ((6, 48), (48, 6), (48, -1), (6, -1), (42, 48), (41, -1), (0, -1)):
        _run(engine, tables, GAS_CC, cells, ta, tb, 0, 3, ("edge", ta, tb))


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_list_lengths_and_where_the_pending_range_starts(engine, tables, n):
    """lists that end before, on and behind a block of 64, the pending ranges of the two tiles starting on and off a block boundary"""
    rng = np.random.default_rng(n)
    cells = [_cell(int(i), int(j)) for i, j in zip(rng.integers(8, 40, n), rng.integers(8, 40, n))]
    for applied_a, applied_b in ((0, 0), (1, 64), (64, 63), (62, n - 1), (n - 1, 0), (64, 64), (min(128, n), 65)):
        _run(engine, tables, NUCLEAR, cells, 2 * COLS + 2, 3 * COLS + 3, min(applied_a, n), min(applied_b, n), ("list", n, applied_a, applied_b))


def test_a_list_beyond_the_on_chip_window(engine, tables):
    """600 generators: the cells of the last 88 come from where the record keeps them, not from LDS"""
    rng = np.random.default_rng(600)
    n = N.ONCHIP_GENS + 88
    cells = [_cell(int(i), int(j)) for i, j in zip(rng.integers(0, GRID, n), rng.integers(0, GRID, n))]
    for applied_a, applied_b in ((500, 512), (511, 513), (512, 0), (576, 448), (n - 1, 520)):
        _run(engine, tables, GAS_CC, cells, 3 * COLS + 3, 3 * COLS + 4, applied_a, applied_b, ("window", applied_a, applied_b))


def test_the_hook_refuses_what_it_cannot_run(engine):
    L = N.lib()
    field = np.zeros(FIELD_DOUBLES)
    fp, out = field.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(0)
    cells = np.array([GRID * GRID], np.uint16)
    cp = cells.ctypes.data_as(C.POINTER(C.c_uint16))
    for args in ((cp, 1, 0, 0, 1), (None, 0, 0, 49, 1), (None, 0, 0, 3, 3), (None, 0, 0, 3, -2), (None, 0, 6, 0, 1), (None, N.MAX_GENS + 1, 0, 0, 1)):
        assert L.eg_debug_tiles_refresh(engine.h, *args, fp, C.byref(out)) == N.EG_ERR_BAD_ARG, args
