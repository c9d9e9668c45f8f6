"""CPU: the host side of build constraints (include/eirgrid_hip.h eg_build_constraints_set) — the struct, what
eg_build_constraints_validate accepts and refuses, the one parser and formatter, and the definition of a build constraint's excess
restated twice (BuildConstraint.excess, and `built_excess_bytes` / `judge_built` below, which the GPU tests import) on hand-made lists
whose answers are written out here.  (The two setters' refusal of a total above 32 needs a context: tests/test_gpu_build_constraints.py.)"""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.constraints import BuildConstraint, Constraint, constraint_list, split_constraints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BYTES = struct.pack("<Q", 0x7FF8000000000000)
NAMES = N.BUILD_CLASS_NAMES


# ---------------------------------------------------------------- the definition, restated (plain Python ints and floats, no numpy arithmetic)
def built_counts(gen_pack, n_gens, off_pack, n_offsets):
    """c[26][19] of one record's lists, by the header's words"""
    c = [[0] * 19 for _ in range(26)]
    for i in range(min(max(int(n_gens), 0), 4096)):
        pk = int(gen_pack[i])
        if (pk & 15) < 15 and ((pk >> 4) & 31) < 26:
            c[(pk >> 4) & 31][pk & 15] += 1
    for i in range(min(max(int(n_offsets), 0), 4096)):
        pk = int(off_pack[i])
        if (pk & 15) < 4 and ((pk >> 4) & 31) < 26:
            c[(pk >> 4) & 31][15 + (pk & 15)] += 1
    return c


def _value(w, m):
    s = 0.0
    for q in range(19):
        s = s + float(w[q]) * float(m[q])
    return s


def built_excess_bytes(counts, c):
    """the eight bytes of build constraint c's excess over one record's counts [26][19], by the header's literal order"""
    b, ge = float(c.bound), c.op == ">="
    if c.aggregate == "sum":
        s = _value(c.weights, [sum(counts[y][q] for y in range(c.from_year, c.to_year)) for q in range(19)])
        e = b - s if ge else s - b
    else:
        x = [b - _value(c.weights, counts[y]) if ge else _value(c.weights, counts[y]) - b for y in range(26)]
        e = x[c.from_year]
        for y in range(c.from_year + 1, c.to_year):
            if e != e:
                continue
            if x[y] != x[y] or x[y] > e:
                e = x[y]
    return NAN_BYTES if e != e else struct.pack("<d", e)


def judge_built(n_gens, gen_pack, n_offsets, off_pack, status, constraints):
    """what the build constraints alone leave for records with these lists and statuses: (violated [n] u32, excess bytes [n][k]); a
    record that did not end EG_EP_OK has mask 0 and a row of NaN"""
    violated, rows = np.zeros(len(status), np.uint32), []
    for j in range(len(status)):
        if status[j] != N.EG_EP_OK:
            rows.append([NAN_BYTES] * len(constraints))
            continue
        counts = built_counts(gen_pack[j], n_gens[j], off_pack[j], n_offsets[j])
        ex = [built_excess_bytes(counts, c) for c in constraints]
        for i, e in enumerate(ex):
            if not struct.unpack("<d", e)[0] <= 0.0:
                violated[j] |= np.uint32(1 << i)
        rows.append(ex)
    return violated, rows


def judge_mixed(yearly, n_gens, gen_pack, n_offsets, off_pack, status, rows_cs, build_cs):
    """judge (tests/test_plan_constraints.py, the row constraints) concatenated with judge_built: (status', violated, excess bytes
    [n][k_rows + k_builds]), the row constraints' bits and columns first"""
    from tests.test_plan_constraints import judge
    out, violated, ex = judge(yearly, status, rows_cs)
    vb, exb = judge_built(n_gens, gen_pack, n_offsets, off_pack, status, build_cs)
    out = np.array(status, np.int32)
    violated = violated | (vb << np.uint32(len(rows_cs)))
    out[(np.asarray(status) == N.EG_EP_OK) & (violated != 0)] = N.EG_EP_INFEASIBLE
    return out, violated, [a + b for a, b in zip(ex, exb)]


def pk(cls, year, mult=0):
    return cls | year << 4 | mult << 9


# ---------------------------------------------------------------- struct and ABI
def test_struct_constants_header_and_exports_agree(built):
    f = N.EgBuildConstraint
    assert C.sizeof(f) == 168
    assert (f.aggregate.offset, f.op.offset, f.from_year.offset, f.to_year.offset, f.pad.offset, f.bound.offset, f.weight.offset) == (0, 1, 2, 3, 4, 8, 16)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert ("typedef struct { uint8_t aggregate, op, from_year, to_year /* 0 <= from < to <= 26 */, pad[4]; double bound /* finite */;\n"
            "                 double weight[EG_BUILD_CLASSES] /* each finite, |w| <= 1e300, not all zero */; } eg_build_constraint; /* 168 bytes */") in header
    for name, value, mine in (("EG_BUILD_CLASSES", "19", N.BUILD_CLASSES), ("EG_BUILD_SPEC_MAX", "1024", N.BUILD_SPEC_MAX)):
        assert re.search(rf"#define {name} {value}(\s|$)", header), name
        assert int(value) == mine, name
    L = N.lib()
    for name in ("eg_build_constraints_validate", "eg_build_constraints_set", "eg_last_batch_build_constraints", "eg_build_constraint_parse",
                 "eg_build_constraint_format", "eg_debug_load_built"):
        assert name in N.EXPORTS and hasattr(L, name), name
        assert len(re.findall(rf"^int32_t {name}\(", header, flags=re.M)) == 1, name
    # the class names are eg_checkpoint.cpp's: kTypeName, then kOffsetName
    src = open(os.path.join(ROOT, "eirgrid_amd", "csrc", "eg_checkpoint.cpp")).read()
    types = re.findall(r'"(\w+)"', re.search(r"kTypeName\[EG_N_TYPES\] = \{(.*?)\};", src, flags=re.S).group(1))
    offsets = re.findall(r'"(\w+)"', re.search(r"kOffsetName\[4\] = \{(.*?)\};", src).group(1))
    assert tuple(types + offsets) == NAMES and len(NAMES) == 19


# ---------------------------------------------------------------- validation
def _raw(**kw):
    s = BuildConstraint({"Nuclear": 1.0}, "<=", 1.0).struct()
    for k, v in kw.items():
        if k.startswith("w"):
            s.weight[int(k[1:])] = v
        else:
            setattr(s, k, v)
    return s


def test_validate_accepts_what_the_definition_allows(built):
    L = N.lib()
    assert L.eg_build_constraints_validate(None, 0) == N.EG_OK
    cs = [BuildConstraint({i % 19: (-1e300 if i & 1 else 1e300), (i + 3) % 19: 0.5}, "<=" if i & 1 else ">=", float(i) - 7.5, i % 26, i % 26 + 1,
                          "sum" if i % 3 else "every") for i in range(32)]
    arr = (N.EgBuildConstraint * 32)(*[c.struct() for c in cs])
    assert L.eg_build_constraints_validate(arr, 32) == N.EG_OK, L.eg_last_error().decode()
    for lo, hi in ((0, 1), (25, 26), (0, 26)):
        arr = (N.EgBuildConstraint * 1)(BuildConstraint({"any": 1.0}, ">=", -1e300, lo, hi).struct())
        assert L.eg_build_constraints_validate(arr, 1) == N.EG_OK


@pytest.mark.parametrize("kw, expect", [
    (dict(aggregate=2), "constraint 1: aggregate 2 (0 EG_AGG_EVERY, 1 EG_AGG_SUM)"),
    (dict(op=2), "constraint 1: op 2 (0 EG_OP_LE, 1 EG_OP_GE)"),
    (dict(from_year=5, to_year=5), "constraint 1: from_year 5 >= to_year 5 (an empty window)"),
    (dict(from_year=9, to_year=3), "constraint 1: from_year 9 >= to_year 3 (an empty window)"),
    (dict(from_year=0, to_year=0), "constraint 1: from_year 0 >= to_year 0 (an empty window)"),
    (dict(to_year=27), "constraint 1: to_year 27 (at most 26)"),
    (dict(bound=float("inf")), "constraint 1: bound inf (a finite number)"),
    (dict(bound=float("-inf")), "constraint 1: bound -inf (a finite number)"),
    (dict(bound=float("nan")), "constraint 1: bound nan (a finite number)"),
    (dict(w7=float("nan")), "constraint 1: weight[7] nan (finite, at most 1e300 in magnitude)"),
    (dict(w0=float("inf")), "constraint 1: weight[0] inf (finite, at most 1e300 in magnitude)"),
    (dict(w18=float("-inf")), "constraint 1: weight[18] -inf (finite, at most 1e300 in magnitude)"),
    (dict(w3=1.0000000000000002e300), "constraint 1: weight[3] 1e+300 (finite, at most 1e300 in magnitude)"),
    (dict(w5=0.0), "constraint 1: weights all zero (at least one class counts)"),
])
def test_validate_names_the_constraint_and_the_field(built, kw, expect):
    L = N.lib()
    arr = (N.EgBuildConstraint * 2)(_raw(), _raw(**kw))
    assert L.eg_build_constraints_validate(arr, 2) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_build_constraints_validate: " + expect


def test_validate_refuses_counts_and_null(built):
    L = N.lib()
    arr = (N.EgBuildConstraint * 1)(_raw())
    for n in (-1, 33):
        assert L.eg_build_constraints_validate(arr, n) == N.EG_ERR_BAD_ARG
        assert L.eg_last_error().decode() == f"eg_build_constraints_validate: n = {n} (0..32)"
    assert L.eg_build_constraints_validate(None, 2) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_build_constraints_validate: NULL constraints with n = 2"
    assert L.eg_build_constraints_set(None, arr, 1) == N.EG_ERR_BAD_ARG and "eg_build_constraints_set: bad argument" in L.eg_last_error().decode()
    assert L.eg_last_batch_build_constraints(None, None) == N.EG_ERR_BAD_ARG
    assert L.eg_debug_load_built(None, None, None, None, None, 1) == N.EG_ERR_BAD_ARG


# ---------------------------------------------------------------- the text form
def _bytes(c):
    return bytes(c.struct())


def test_the_issue_examples_parse_to_what_they_say(built):
    w = lambda **kw: tuple(float(kw.get(n, 0.0)) for n in NAMES)      # noqa: E731
    assert BuildConstraint.parse("built(GasPeaker + GasCombinedCycle) <= 0") == BuildConstraint(w(GasPeaker=1, GasCombinedCycle=1), "<=", 0.0)
    assert BuildConstraint.parse("sum(built(Nuclear)) <= 2") == BuildConstraint(w(Nuclear=1), "<=", 2.0, 0, 26, "sum")
    assert BuildConstraint.parse("built(OnshoreWind) <= 4 @2025:2034") == BuildConstraint(w(OnshoreWind=1), "<=", 4.0, 0, 10)
    assert BuildConstraint.parse("sum(built(BatteryStorage - OnshoreWind)) >= 0 @2025:2035") == \
        BuildConstraint(w(BatteryStorage=1, OnshoreWind=-1), ">=", 0.0, 0, 11, "sum")
    assert BuildConstraint.parse("sum(built(CarbonCredit)) <= 10") == BuildConstraint(w(CarbonCredit=1), "<=", 10.0, 0, 26, "sum")
    # any, signed and fractional weights, windows, spacing
    assert BuildConstraint.parse("built(any) <= 3").weights == (1.0,) * 15 + (0.0,) * 4
    assert BuildConstraint.parse("built(2.5*any - 0.5*Forest)>=1e3 @2030") == BuildConstraint((2.5,) * 15 + (-0.5, 0.0, 0.0, 0.0), ">=", 1000.0, 5, 26)
    assert BuildConstraint.parse("built(-1*OnshoreWind+1e+2*Nuclear-3.25*Wetland) <= -0.5 @2050") == \
        BuildConstraint(w(OnshoreWind=-1, Nuclear=100, Wetland=-3.25), "<=", -0.5, 25, 26)
    assert BuildConstraint.parse("built(BatteryStorage-OnshoreWind) <= 0") == BuildConstraint(w(BatteryStorage=1, OnshoreWind=-1), "<=", 0.0)
    assert BuildConstraint.parse("  sum( built( 3 * any ) )  <=  1  @2026:2026 ") == BuildConstraint((3.0,) * 15 + (0.0,) * 4, "<=", 1.0, 1, 2, "sum")
    # the formatter: index order, 17 digits for what is not 1, `any` only for equal generator weights and no offsets
    assert str(BuildConstraint.parse("built(GasPeaker + GasCombinedCycle) <= 0")) == "built(GasCombinedCycle + GasPeaker) <= 0"
    assert str(BuildConstraint.parse("sum(built(BatteryStorage - OnshoreWind)) >= 0 @2025:2035")) == "sum(built(-1*OnshoreWind + BatteryStorage)) >= 0 @2025:2035"
    assert str(BuildConstraint((0.1,) * 15 + (0.0,) * 4, "<=", 0.3, 3, 26)) == "built(0.10000000000000001*any) <= 0.29999999999999999 @2028"
    assert str(BuildConstraint({"any": 1.0}, ">=", 2.0)) == "built(any) >= 2"
    assert str(BuildConstraint({"any": 1.0, "Forest": -0.5}, ">=", 2.0)).startswith("built(OnshoreWind + OffshoreWind + ") and \
        str(BuildConstraint({"any": 1.0, "Forest": -0.5}, ">=", 2.0)).endswith("+ WaveEnergy - 0.5*Forest) >= 2")


def test_parse_of_format_is_the_constraint_byte_for_byte(built):
    rng = np.random.default_rng(7)
    pool = np.array([0.0, 0.0, 1.0, -1.0, 0.5, 3.25, 1e300, -1e300, 0.1, 1 / 3, 5e-324, 123456789.125])
    for i in range(400):
        w = rng.choice(pool, 19)
        if i % 4 == 0:
            w = rng.normal(0.0, 1e3, 19) * (rng.random(19) < 0.5) + 0.0      # (+ 0.0: no -0.0, the one weight that reads back as +0.0)
        if i % 9 == 0:
            w = np.array([rng.choice(pool[2:])] * 15 + [0.0] * 4)      # `any`
        if not w.any():
            w[int(rng.integers(0, 19))] = 1.0
        lo = int(rng.integers(0, 26)); hi = 26 if i % 3 == 0 else int(rng.integers(lo + 1, 27))
        c = BuildConstraint(tuple(w), "<=" if i & 1 else ">=", float(rng.choice([0.0, 2.0, -7.5, 1e-300, 1.7976931348623157e308, rng.normal()])), lo, hi,
                            "sum" if i % 5 < 2 else "every")
        text = str(c)
        back = BuildConstraint.parse(text)
        assert _bytes(back) == _bytes(c), (text, c)
        assert len(text) < N.BUILD_SPEC_MAX and ("any" in text) == (len(set(w[:15])) == 1 and w[0] != 0 and not w[15:].any()), text


def test_a_weight_of_minus_zero_reads_back_as_plus_zero(built):
    c = BuildConstraint({"Nuclear": 1.0, "Forest": -0.0}, "<=", 1.0)
    assert str(c) == "built(Nuclear) <= 1" and _bytes(BuildConstraint.parse(str(c))) == _bytes(BuildConstraint({"Nuclear": 1.0}, "<=", 1.0)) != _bytes(c)


@pytest.mark.parametrize("spec, expect", [
    ("", 'an empty constraint ("[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]")'),
    ("   ", 'an empty constraint ("[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]")'),
    ("net_co2 <= 0", 'expected "built(", found "net_co2" in "net_co2 <= 0" ("[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]")'),
    ("built(Gas) <= 0", 'unknown class "Gas" in "built(Gas) <= 0" (a generator type — OnshoreWind, GasPeaker, Nuclear, ... —, Forest, Wetland, ActiveCapture, '
                        'CarbonCredit or any)'),
    ("built() <= 0", 'unknown class "" in "built() <= 0" (a generator type — OnshoreWind, GasPeaker, Nuclear, ... —, Forest, Wetland, ActiveCapture, CarbonCredit or any)'),
    ("built(nuclear) <= 0", 'unknown class "nuclear" in "built(nuclear) <= 0" (a generator type — OnshoreWind, GasPeaker, Nuclear, ... —, Forest, Wetland, '
                            'ActiveCapture, CarbonCredit or any)'),
    ("built(Nuclear + Nuclear) <= 0", 'class "Nuclear" is named twice in "built(Nuclear + Nuclear) <= 0"'),
    ("built(any - 2*GasPeaker) <= 0", 'class "GasPeaker" is named twice in "built(any - 2*GasPeaker) <= 0"'),
    ("built(Biomass + any) <= 0", 'class "Biomass" is named twice in "built(Biomass + any) <= 0" (any names every generator type)'),
    ("built(x*Nuclear) <= 0", 'weight "x" is not a number'),
    ("built(1e301*Nuclear) <= 0", 'weight "1e301" (finite, at most 1e300 in magnitude)'),
    ("built(nan*Nuclear) <= 0", 'weight "nan" (finite, at most 1e300 in magnitude)'),
    ("built(0*Nuclear) <= 0", 'weights all zero (at least one class counts) in "built(0*Nuclear) <= 0"'),
    ("built(Nuclear Forest) <= 0", 'expected "+", "-" or ")" behind a class, found "Forest)" in "built(Nuclear Forest) <= 0"'),
    ("built(Nuclear) < 0", 'expected "<=" or ">=" behind "built(...)", found "<"'),
    ("built(Nuclear) = 0", 'expected "<=" or ">=" behind "built(...)", found "="'),
    ("sum(built(Nuclear) <= 0", 'expected ")" behind "sum(built(...)", found "<= 0"'),
    ("built(Nuclear) <= zero", 'bound "zero" is not a number'),
    ("built(Nuclear) <=", 'bound "" is not a number'),
    ("built(Nuclear) <= inf", 'bound "inf" is not finite'),
    ("built(Nuclear) <= 0 @2024", 'year "2024" (a calendar year 2025..2050)'),
    ("built(Nuclear) <= 0 @2030:2051", 'year "2051" (a calendar year 2025..2050)'),
    ("built(Nuclear) <= 0 @2030:2029", 'window "2030:2029" ends before it starts'),
    ("built(Nuclear) <= 0 extra", 'unexpected "extra" behind the constraint in "built(Nuclear) <= 0 extra"'),
])
def test_parse_errors_quote_the_offending_token(built, spec, expect):
    L = N.lib()
    s = N.EgBuildConstraint()
    assert L.eg_build_constraint_parse(spec.encode(), C.byref(s)) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_build_constraint_parse: " + expect
    assert L.eg_build_constraint_parse(None, C.byref(s)) == N.EG_ERR_BAD_ARG and L.eg_build_constraint_parse(b"built(any) <= 1", None) == N.EG_ERR_BAD_ARG


def test_format_refuses_a_bad_constraint_and_a_short_buffer(built):
    L = N.lib()
    buf = C.create_string_buffer(N.BUILD_SPEC_MAX)
    bad = _raw(to_year=27)
    assert L.eg_build_constraint_format(C.byref(bad), buf, len(buf)) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_build_constraint_format: to_year 27 (at most 26)"
    # the longest spec: 19 weights and a bound of 24 characters each, both wrappers, a two-year window
    longest = BuildConstraint((-1.2345678901234567e299,) * 14 + (-1.2345678901234566e299,) + (-1.2345678901234567e299,) * 4, ">=", -1.7976931348623157e308, 1, 25, "sum")
    s = longest.struct()
    assert L.eg_build_constraint_format(C.byref(s), buf, len(buf)) == N.EG_OK
    text = buf.value.decode()
    # 19 x ("-1.2345678901234567e+299" or its " - " form + "*" + the name), "sum(built(" .. "))", " >= ", the bound, " @2026:2049"
    assert len(text) == sum(len(n) for n in NAMES) + 19 * (23 + 1) + 1 + 18 * 3 + 10 + 2 + 4 + 24 + 11 and len(text) + 1 <= N.BUILD_SPEC_MAX
    assert BuildConstraint.parse(text) == longest
    for short in (1, len(text) // 2, len(text)):      # one byte short of the text and its terminator, and shorter
        assert L.eg_build_constraint_format(C.byref(s), C.create_string_buffer(short), short) == N.EG_ERR_BAD_ARG
        assert L.eg_last_error().decode() == f"eg_build_constraint_format: the buffer holds {short} bytes ({len(text) + 1} needed)"
    exact = C.create_string_buffer(len(text) + 1)
    assert L.eg_build_constraint_format(C.byref(s), exact, len(exact)) == N.EG_OK and exact.value.decode() == text
    assert L.eg_build_constraint_format(C.byref(s), buf, 0) == N.EG_ERR_BAD_ARG and L.eg_build_constraint_format(None, buf, 8) == N.EG_ERR_BAD_ARG


def test_a_mixed_list_keeps_its_order_and_refuses_rows_behind_builds(built):
    cs = constraint_list(["net_co2 <= 0 @2040", Constraint("balance", ">=", 1.0), "sum(built(Nuclear)) <= 2", BuildConstraint({"any": 1.0}, "<=", 9.0)])
    assert [type(c) for c in cs] == [Constraint, Constraint, BuildConstraint, BuildConstraint]
    rows, builds = split_constraints(cs)
    assert rows == cs[:2] and builds == cs[2:]
    assert split_constraints(["built(any) <= 1"]) == ([], [BuildConstraint({"any": 1.0}, "<=", 1.0)]) and split_constraints(None) == ([], [])
    with pytest.raises(ValueError, match=r"constraint 1 \(balance >= 1\) is a row constraint behind a build constraint \(built\(any\) <= 1\)"):
        split_constraints(["built(any) <= 1", "balance >= 1"])
    assert [str(c) for c in cs] == ["net_co2 <= 0 @2040", "balance >= 1", "sum(built(Nuclear)) <= 2", "built(any) <= 9"]      # what the scripts' CSV headers print
    with pytest.raises(ValueError, match="unknown class 'Gas'"):
        BuildConstraint({"Gas": 1.0}, "<=", 0.0)
    with pytest.raises(ValueError, match=r"18 weights \(19: one per class\)"):
        BuildConstraint((1.0,) * 18, "<=", 0.0)


# ---------------------------------------------------------------- the definition on hand-made lists, the answers written out
NUC, WIND, BAT, GAS = NAMES.index("Nuclear"), NAMES.index("OnshoreWind"), NAMES.index("BatteryStorage"), NAMES.index("GasPeaker")


def _lists(gens=(), offs=(), n_gens=None, n_offsets=None, fill=0):
    g, o = np.full(4096, fill, np.uint16), np.full(4096, fill, np.uint16)
    g[:len(gens)] = gens; o[:len(offs)] = offs
    return g, (len(gens) if n_gens is None else n_gens), o, (len(offs) if n_offsets is None else n_offsets)


def _both(c, lists):
    """the excess by BuildConstraint.excess, checked against built_excess_bytes over built_counts and BuildConstraint.counts"""
    g, ng, o, no = lists
    counts = built_counts(g, ng, o, no)
    assert BuildConstraint.counts(g, ng, o, no).tolist() == counts
    e = c.excess(g, ng, o, no)
    assert struct.pack("<d", e) == built_excess_bytes(counts, c), (c, e)
    assert c.violated(g, ng, o, no) == (not e <= 0.0)
    assert judge_built([ng], [g], [no], [o], [0], [c]) == (np.array([0 if e <= 0.0 else 1], np.uint32), [[struct.pack("<d", e)]])
    return e


def test_the_excess_on_hand_made_lists(built):
    nuclear = lambda **kw: BuildConstraint({"Nuclear": 1.0}, **kw)      # noqa: E731
    # an empty list: every count 0, the value +0.0
    empty = _lists()
    assert _both(nuclear(op="<=", bound=0.0), empty) == 0.0 and _both(nuclear(op="<=", bound=2.0, aggregate="sum"), empty) == -2.0
    assert _both(nuclear(op=">=", bound=1.0), empty) == 1.0 and _both(BuildConstraint({"Nuclear": -1.0}, "<=", 0.0), empty) == 0.0
    assert struct.pack("<d", _both(BuildConstraint({"Nuclear": -1.0}, ">=", 0.0), empty)) == struct.pack("<d", 0.0)      # +0.0 + -0.0 is +0.0: bound - s = +0.0
    # one entry in the window's first and in its last year; one just outside either end
    for year, inside in ((4, False), (5, True), (9, True), (10, False)):
        one = _lists([pk(NUC, year, 2)])
        assert _both(nuclear(op="<=", bound=0.0, from_year=5, to_year=10), one) == (1.0 if inside else 0.0), year
        assert _both(nuclear(op="<=", bound=0.0, from_year=5, to_year=10, aggregate="sum"), one) == (1.0 if inside else 0.0), year
    # an entry in year index 26 and one in 31: counted nowhere
    late = _lists([pk(NUC, 26), pk(NUC, 31), pk(NUC, 25)])
    assert np.array(built_counts(*late)).sum() == 1 and _both(nuclear(op="<=", bound=0.0, aggregate="sum"), late) == 1.0
    # class nibble 15 among the generators, offset nibble 4 and above: counted nowhere; offset nibbles 0..3 are classes 15..18
    odd = _lists([pk(15, 3), pk(14, 3)], [pk(4, 3), pk(15, 3), pk(3, 3), pk(0, 3), pk(3, 4)])
    c = built_counts(*odd)
    assert sum(map(sum, c)) == 4 and c[3][14] == 1 and c[3][18] == 1 and c[3][15] == 1 and c[4][18] == 1
    assert _both(BuildConstraint({"CarbonCredit": 1.0}, "<=", 10.0, aggregate="sum"), odd) == -8.0
    assert _both(BuildConstraint({"any": 1.0, "Forest": 1.0, "Wetland": 1.0, "ActiveCapture": 1.0, "CarbonCredit": 1.0}, "<=", 0.0, aggregate="sum"), odd) == 4.0
    # garbage behind n_gens is never data
    junk = _lists([pk(NUC, 1), pk(NUC, 2)], fill=pk(NUC, 2))
    assert _both(nuclear(op="<=", bound=0.0, aggregate="sum"), junk) == 2.0 and _both(nuclear(op="<=", bound=0.0), junk) == 1.0
    assert _both(BuildConstraint({"Forest": 1.0}, "<=", 0.0, aggregate="sum"), junk) == 0.0      # (the offsets' fill is Forest in year 2 — behind n_offsets = 0)
    # n_gens of -1 (nothing) and 5 000 (the whole list, 4 096 entries)
    full = np.full(4096, pk(NUC, 7), np.uint16)
    assert _both(nuclear(op="<=", bound=0.0, aggregate="sum"), (full, -1, full, -1)) == 0.0
    assert _both(nuclear(op="<=", bound=0.0, aggregate="sum"), (full, 5000, full, 5000)) == 4096.0
    assert _both(BuildConstraint({"Forest": 0.5}, "<=", 0.0), (full, 5000, full, 5000)) == 0.0      # (offset nibble 5: no class)
    # EVERY against SUM on the same counts: wind 3, 1, 2 in the years 2, 3, 4
    wind = _lists([pk(WIND, 2)] * 3 + [pk(WIND, 3)] + [pk(WIND, 4)] * 2 + [pk(BAT, 3)] * 4)
    assert _both(BuildConstraint({"OnshoreWind": 1.0}, "<=", 4.0), wind) == -1.0 and _both(BuildConstraint({"OnshoreWind": 1.0}, "<=", 4.0, aggregate="sum"), wind) == 2.0
    assert _both(BuildConstraint({"OnshoreWind": 1.0}, ">=", 1.0, 2, 5), wind) == 0.0 and _both(BuildConstraint({"OnshoreWind": 1.0}, ">=", 1.0, 2, 5, "sum"), wind) == -5.0
    assert _both(BuildConstraint({"BatteryStorage": 1.0, "OnshoreWind": -1.0}, ">=", 0.0, aggregate="sum"), wind) == 2.0       # 4 batteries, 6 farms
    assert _both(BuildConstraint({"BatteryStorage": 1.0, "OnshoreWind": -1.0}, ">=", 0.0), wind) == 3.0                         # year 2: 0 - 3
    assert _both(BuildConstraint({"BatteryStorage": 0.5, "OnshoreWind": 3.25}, "<=", 5.0, 3, 4), wind) == 0.25                  # 3.25 + 2.0 - 5
    # a tie of two years (1 and 5 both exceed by 1: the first stands, the second does not move it)
    tie = _lists([pk(GAS, 1), pk(GAS, 5)])
    assert _both(BuildConstraint({"GasPeaker": 1.0}, "<=", 0.0), tie) == 1.0
    # value exactly on the bound: satisfied, excess +0.0, and one build more violates by exactly the weight
    on = _lists([pk(NUC, 3), pk(NUC, 9)])
    assert _both(nuclear(op="<=", bound=2.0, aggregate="sum"), on) == 0.0 and not nuclear(op="<=", bound=2.0, aggregate="sum").violated(*on)
    assert _both(nuclear(op=">=", bound=2.0, aggregate="sum"), on) == 0.0 and _both(nuclear(op="<=", bound=1.0, aggregate="sum"), on) == 1.0
    assert _both(BuildConstraint({"Nuclear": 1e300}, "<=", 2e300, aggregate="sum"), on) == 0.0
    assert _both(BuildConstraint({"Nuclear": 1e300, "Forest": -1e300}, "<=", 0.0, aggregate="sum"), _lists([pk(NUC, 3)], [pk(0, 4)])) == 0.0


def test_the_first_of_equal_years_wins_and_the_order_of_the_classes_is_the_definitions(built):
    # the class order shows in the rounding: 1e300 - 1e300 + 1 is 1, 1 + 1e300 - 1e300 is 0
    a = BuildConstraint({0: 1e300, 1: -1e300, 2: 1.0}, "<=", 0.0)
    b = BuildConstraint({0: 1.0, 1: 1e300, 2: -1e300}, "<=", 0.0)
    lists = _lists([pk(0, 0), pk(1, 0), pk(2, 0)])
    assert _both(a, lists) == 1.0 and _both(b, lists) == 0.0
    # the first of equal years wins, by the sign of zero: -0.0 and +0.0 are equal, so the +0.0 of year 0 stands against the -0.0 of year 1
    z = BuildConstraint({"GasPeaker": 1.0}, "<=", 1.0, 0, 2)      # year 0: 1 - 1 = +0.0
    assert struct.pack("<d", _both(z, _lists([pk(GAS, 0), pk(GAS, 1)]))) == struct.pack("<d", 0.0)
    z = BuildConstraint({"GasPeaker": -1.0}, "<=", 0.0, 0, 2)      # year 0: (+0.0 + -1.0) - 0 = -1; year 1: no build, +0.0 + -0.0 = +0.0: the larger
    assert struct.pack("<d", _both(z, _lists([pk(GAS, 0)]))) == struct.pack("<d", 0.0)
    # the fold over the years follows the row rule: the largest, and on a tie nothing moves
    c = BuildConstraint({"GasPeaker": 1.0}, ">=", 1.0, 2, 6)
    assert _both(c, _lists([pk(GAS, 2), pk(GAS, 4), pk(GAS, 4)])) == 1.0      # years 3 and 5 both miss by 1
