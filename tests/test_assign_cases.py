"""The cases and the restatement of pairing by assignment (tests/assign_cases.py) on the CPU: every decision keeps
match_cases.MARGIN from its bound in float64, every winner's assignment is unique by a cost gap above it, the
shortest-augmenting-path solver equals brute force (and scipy, where installed), the float32 restatement agrees with
float64 on every integer field, and the three option classes validate `pairing`."""

import itertools

import numpy as np
import pytest

from chemeleon_amd.match import Match, Reference
from chemeleon_amd.match_group import MatchDedup
from chemeleon_amd.match_set import MatchSet, ReferenceSet
from tests import assign_cases as A
from tests import match_cases as M


def by_name(name):
    return next(g for g, c in enumerate(A.cases()) if c["name"] == name)


def test_every_decision_keeps_the_margin():
    for c, r in zip(A.cases(), A.reference("float64")):
        for f in ("lattice_margin", "thin_margin", "pair_margin", "gap_margin", "rms_margin"):
            assert r[f] > M.MARGIN, (c["name"], f, r[f])
        assert r["matched"] == c["matched"], c["name"]
        assert r["flags"] == c["flags"], c["name"]


def test_every_winners_assignment_is_unique():
    collided = 0
    for c, r in zip(A.cases(), A.reference("float64")):
        if r["matched"] and r["collided"]:
            collided += 1
            assert r["assign_gap"] > M.MARGIN, (c["name"], r["assign_gap"])
            n = len(r["perm"])
            assert sorted(r["perm"].tolist()) == list(range(n))
            assert np.array_equal(c["sample"]["types"][r["perm"]], c["ref"]["types"])
    assert collided >= 8


def test_what_the_cases_are_for():
    ref = A.reference("float64")
    three = ref[by_name("three")]
    assert three["matched"] == 1 and three["collided"] and abs(three["rms"] - 0.077) < 1e-3
    assert three["nearest"]["matched"] == 0 and three["nearest"]["n_survivors"] == 0 and three["n_candidates"] == 16
    assert ref[by_name("chain")]["longest_path"] >= 3          # two placed rows are placed again
    assert 4 < ref[by_name("symmetric16")]["n_assigned"] <= A.MAX_ASSIGN
    many = ref[by_name("many")]
    assert many["flags"] == A.MANY_ASSIGNMENTS and many["n_assigned"] == A.MAX_ASSIGN < many["n_survivors"]
    assert ref[by_name("moved1")]["n_survivors"] == 0
    nan = ref[by_name("nan")]
    assert nan["matched"] == 0 and nan["n_assigned"] > 0      # alive and collided, and the solve finds no column
    for name in ("rutile_collided", "rocksalt8_collided"):    # two species blocks, the collided one at an offset
        c = A.cases()[by_name(name)]
        assert len(set(c["ref"]["types"].tolist())) == 2 and ref[by_name(name)]["n_assigned"] > 0
    assert [len(A.cases()[by_name(f"sc_{n}_collided")]["ref"]["types"]) for n in (63, 64, 65, 256)] == [63, 64, 65, 256]


def _blocks(rng, sizes):
    types = np.repeat(np.arange(len(sizes)), sizes)
    n = len(types)
    return rng.random((n, n)) ** 2, types[:, None] == types[None, :], types


def test_solver_equals_brute_force():
    rng = np.random.default_rng(7)
    for sizes in [(1,), (2,), (3, 1), (1, 4), (5, 2), (7,), (3, 3, 1), (6, 1)] * 6:
        cost, same, types = _blocks(rng, sizes)
        if rng.random() < 0.5:  # many ties in the row minima: every row wants column 0 of its block
            cost[:, np.flatnonzero(np.r_[True, np.diff(types) != 0])] *= 0.01
        col, _ = A.solve(cost, same)
        assert np.all(same[np.arange(len(col)), col]) and sorted(col.tolist()) == list(range(len(col)))
        best, first = 0.0, 0
        for size in sizes:
            rows = np.arange(first, first + size)
            best += min(cost[rows, first + np.array(p)].sum() for p in itertools.permutations(range(size)))
            first += size
        assert abs(cost[np.arange(len(col)), col].sum() - best) <= 1e-12, sizes


def test_solver_equals_scipy():
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(8)
    for n in (2, 9, 40, 130):
        cost, same, _ = _blocks(rng, (n,))
        col, _ = A.solve(cost, same)
        r, c = optimize.linear_sum_assignment(cost)
        assert abs(cost[np.arange(n), col].sum() - cost[r, c].sum()) <= 1e-10


def test_solver_gives_up_on_nan_and_inf():
    same = np.ones((3, 3), dtype=bool)
    cost = np.array([[1.0, 2.0, np.nan], [1.5, 0.5, np.nan], [0.2, 0.1, np.nan]])
    assert A.solve(cost, same) is None
    cost[:, 2] = np.inf
    assert A.solve(cost, same) is None
    assert A.solve(np.full((2, 2), np.nan), same[:2, :2]) is None


def test_float32_agrees_on_the_integer_fields():
    for c, a, b in zip(A.cases(), A.reference("float32"), A.reference("float64")):
        for f in A.INT_FIELDS:
            assert a[f] == b[f], (c["name"], f, a[f], b[f])
    err = A.float32_error()
    print("float32 restatement against float64:", err)
    assert 16 * err < 1e-3 * M.STOL


def test_pairing_is_validated_on_the_host():
    c = A.cases()[0]
    ref = Reference.from_arrays(*M.packed([c["ref"]]))
    known = ReferenceSet.from_arrays(*M.packed([c["ref"]]))
    for make in (lambda **k: Match(ref, **k), lambda **k: MatchDedup(**k), lambda **k: MatchSet(known, **k)):
        assert make().pairing == "nearest" and make(pairing="assignment").pairing == "assignment"
        for bad in ("optimal", "", None, 1, b"nearest", "Nearest"):
            with pytest.raises(ValueError, match="pairing"):
                make(pairing=bad)
