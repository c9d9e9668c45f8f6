"""CPU: one grammar behind the two constraint parsers (csrc/eg_constraint_text.cpp eg_plan_constraint_parse, eg_build_constraint_parse).  A
row constraint and a build constraint differ in their head — a column, or built(...) —; the aggregate around it and everything behind it,
"(<=|>=) BOUND [@FROM[:TO]]", is the same text form.  Every tail of a fixed list goes behind a head of either kind: both parsers accept it
with equal fields, or both refuse it with the same message once the entry point's name and the head's text are taken out.  What either
formatter writes for an accepted constraint parses back to the same bytes."""
import ctypes as C
import struct

import pytest

from eirgrid_amd import _native as N

# (the row head, the build head): plain, under sum(), under sum() with blanks
HEADS = [("net_co2", "built(Nuclear)"), ("sum(net_co2)", "sum(built(Nuclear))"), ("sum( net_co2 )", "sum( built( Nuclear ) )")]
TAILS = ["<= 1", ">= -2.5e3 @2030", "<= 0 @2030:2039", "<=0@2050", "<=0@2025:2050", "< 1", "<= abc", "<= inf", "<= nan", "<= 1e999", "<= 0x10",
         "<= 1 @2024", "<= 1 @2051", "<= 1 @2030:2029", "<= 1 @2030:", "<= 1 @", "<= 1 @20x0", "<= 1 @2030:2031:2032", "<= 1 junk",
         "<= 1 @2030 junk", "<=", "", "= 1", "=> 1", "<= 1 @2030 : 2031", "\t>=\t7\t@2031:2040\t", "<= -0.0", "<= 1.", "<= +1"]
# the one pair with a parenthesis missing
UNCLOSED = ("sum(net_co2", "sum(built(Nuclear)")

KINDS = (("eg_plan_constraint_parse", "eg_plan_constraint_format", N.EgPlanConstraint, N.CONSTRAINT_SPEC_MAX),
         ("eg_build_constraint_parse", "eg_build_constraint_format", N.EgBuildConstraint, N.BUILD_SPEC_MAX))


def _parse(kind, head, tail):
    """(the struct, None) or (None, the message without the entry point's name and with the head's text as one token)"""
    parse, _, ctype, _ = KINDS[kind]
    L, s = N.lib(), ctype()
    if getattr(L, parse)((head + " " + tail).encode(), C.byref(s)) == N.EG_OK:
        return s, None
    msg = L.eg_last_error().decode()
    assert msg.startswith(parse + ": "), msg
    msg = msg[len(parse) + 2:]
    for text in (head, "sum(net_co2", "sum(built(...)", "built(...)", "net_co2"):
        msg = msg.replace(text, "HEAD")
    return None, msg


def _tail_fields(s):
    return s.aggregate, s.op, s.from_year, s.to_year, struct.pack("<d", s.bound)


def _round_trip(kind, s):
    parse, fmt, ctype, spec_max = KINDS[kind]
    L, buf, back = N.lib(), C.create_string_buffer(spec_max), ctype()
    assert getattr(L, fmt)(C.byref(s), buf, len(buf)) == N.EG_OK, L.eg_last_error().decode()
    assert getattr(L, parse)(buf.value, C.byref(back)) == N.EG_OK, (buf.value, L.eg_last_error().decode())
    assert bytes(back) == bytes(s), buf.value


@pytest.mark.parametrize("heads", HEADS, ids=["plain", "sum", "sum-blanks"])
def test_a_tail_means_the_same_behind_either_head(built, heads):
    accepted = 0
    for tail in TAILS:
        (row, row_msg), (build, build_msg) = _parse(0, heads[0], tail), _parse(1, heads[1], tail)
        assert (row is None) == (build is None), (tail, row_msg, build_msg)
        if row is None:
            assert row_msg == build_msg, tail
            continue
        accepted += 1
        assert _tail_fields(row) == _tail_fields(build), tail
        assert row.aggregate == (N.AGG_SUM if heads[0].startswith("sum(") else N.AGG_EVERY), tail
        _round_trip(0, row)
        _round_trip(1, build)
    assert 0 < accepted < len(TAILS)      # (the list holds both: "<= 1" is a constraint, "< 1" is none)


def test_a_missing_parenthesis_is_refused_alike(built):
    (row, row_msg), (build, build_msg) = _parse(0, UNCLOSED[0], "<= 1"), _parse(1, UNCLOSED[1], "<= 1")
    assert row is None and build is None
    assert row_msg == build_msg == 'expected ")" behind "HEAD", found "<= 1"'
