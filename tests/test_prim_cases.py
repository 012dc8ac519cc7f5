"""The primitive-cell cases and their two numpy restatements (tests/prim_cases.py) against each other and against
the textbook, without a GPU: the conditions under which the device test (tests/test_gpu_primitive.py) may pin the
kernels to the float32 restatement bit for bit, and the host-side validation of chemeleon_amd.Primitive."""

import numpy as np
import pytest

from tests import prim_cases as P
from tests import symmetry_cases as S

NAMED = tuple(P.EXPECTED) + ("one_halving", "prim_halving", "thin", "no_lattice")


def both():
    return list(zip(P.cases(), P.reference("float32"), P.reference("float64")))


def test_the_conditions_on_the_cases_hold():
    names = [c["name"] for c in P.cases()]
    assert len(set(names)) == len(names)
    for name in NAMED:  # none of the named cases may be dropped
        assert name in names, name
    families = {c["family"] for c in P.cases()}
    assert len(P.dropped_variants()) <= 0.05 * len(names), P.dropped_variants()
    for d in P.dropped_variants():  # (dropped variants are listed; a family never loses its base case)
        assert d.rsplit("_v", 1)[0] in families
    for c, r32, r64 in both():
        assert min(r64["margin"], r64["lattice_margin"]) >= P.MARGIN, (c["name"], r64["margin"], r64["lattice_margin"])
        assert not r64["flags"] & P.AMBIGUOUS and not r32["flags"] & P.AMBIGUOUS, c["name"]
    assert P.find_halving() == P.HALVING


def test_float32_and_float64_agree_on_every_integer_field():
    for c, r32, r64 in both():
        for f in P.INT_FIELDS + ("lattice_system",):
            assert r32[f] == r64[f], (c["name"], f, r32[f], r64[f])
        assert r32["tol"] == r64["tol"] and r32["H"] == r64["H"], c["name"]
        np.testing.assert_array_equal(r32["keep"], r64["keep"], err_msg=c["name"])
        np.testing.assert_array_equal(r32["Lp"].view(np.uint32), r64["Lp"].view(np.uint32), err_msg=c["name"])
        np.testing.assert_array_equal(r32["xp"].view(np.uint32), r64["xp"].view(np.uint32), err_msg=c["name"])


def test_textbook_sizes():
    for c, r32, _ in both():
        if c["family"] in P.EXPECTED:
            n, n_prim, m = P.EXPECTED[c["family"]]
            assert (len(c["types"]), r32["n_prim"], r32["n_trans"]) == (n, n_prim, m), c["name"]
            assert r32["flags"] == 0 and r32["halvings"] == 0, c["name"]
            assert len(r32["xp"]) == n_prim and len(r32["types_p"]) == n_prim
    by = {c["name"]: r for c, r, _ in both()}
    assert by["prim_halving"]["halvings"] >= 1 and by["prim_halving"]["flags"] == 0
    assert by["one_halving"]["flags"] == 0 and by["one_halving"]["n_prim"] == 8
    assert by["thin"]["flags"] == P.THIN and by["thin"]["tol"] == np.float32(P.SYMPREC) and by["thin"]["n_prim"] == 1
    assert by["no_lattice"]["flags"] == P.NO_LATTICE and by["no_lattice"]["n_prim"] == 2
    assert by["no_lattice"]["lattice_system"] == -1
    H = by["rocksalt8"]["H"]
    assert H[0][1] or H[0][2] or H[1][2]  # the fcc centring: H is not diagonal


def test_hermite_normal_form_conditions():
    for c, r32, _ in both():
        H, m = r32["H"], r32["n_trans"]
        assert H[1][0] == H[2][0] == H[2][1] == 0 and min(H[0][0], H[1][1], H[2][2]) > 0, c["name"]
        assert 0 <= H[0][1] < H[1][1] and 0 <= H[0][2] < H[2][2] and 0 <= H[1][2] < H[2][2], c["name"]
        if r32["n_prim"] < len(c["types"]):
            assert H[0][0] * H[1][1] * H[2][2] == m * m, c["name"]
            for k in range(3):  # m e_k lies in the lattice of H: m adj(H) / det(H) = adj(H) / m is integral
                assert all(v % m == 0 for v in P.adjugate(H)[k]), c["name"]
        else:
            assert H == [[1, 0, 0], [0, 1, 0], [0, 0, 1]], c["name"]
    # the normal form itself: unique under any order and any unimodular mixing of the generators
    rng = np.random.default_rng(3)
    for _ in range(50):
        m = int(rng.integers(1, 12))
        gens = [list(map(int, rng.integers(0, m, 3))) for _ in range(int(rng.integers(0, 5)))]
        full = gens + [[m, 0, 0], [0, m, 0], [0, 0, m]]
        H = P.hnf(full)
        mixed = [[a + 2 * b for a, b in zip(full[k], full[k - 1])] for k in rng.permutation(len(full))] + full[:1]
        assert P.hnf(mixed) == H and P.hnf(list(reversed(full))) == H


def test_volume_and_expansion_reproduce_the_supercell():
    for c, r32, _ in both():
        n, m = len(c["types"]), r32["n_trans"]
        if r32["n_prim"] == n:
            np.testing.assert_array_equal(r32["Lp"], r32["Lr"])
            np.testing.assert_array_equal(r32["xp"].view(np.uint32), r32["xr"].view(np.uint32))
            continue
        Lr, Lp = r32["Lr"].astype(np.float64), r32["Lp"].astype(np.float64)
        vr, vp = abs(np.linalg.det(Lr)), abs(np.linalg.det(Lp))
        assert abs(vp * m - vr) <= 1e-5 * vr, (c["name"], vp, vr)
        assert np.linalg.det(Lp) * np.linalg.det(Lr) > 0  # the handedness is kept
        assert np.all((r32["xp"] >= 0) & (r32["xp"] < 1))
        # every atom of the supercell is a kept atom plus a vector of the primitive lattice, within tol; every
        # kept atom stands for exactly m of them
        cart = r32["xr"].astype(np.float64) @ Lr
        prim = r32["xp"].astype(np.float64) @ Lp
        np.testing.assert_array_equal(r32["types_p"], c["types"][r32["keep"]])
        d = (cart[:, None, :] - prim[None, :, :]) @ np.linalg.inv(Lp)
        d -= np.rint(d)
        dist = np.linalg.norm(d @ Lp, axis=-1)
        dist[c["types"][:, None] != r32["types_p"][None, :]] = np.inf
        hit = dist <= float(r32["tol"]) * (1 + P.MARGIN)
        assert hit.any(axis=1).all(), c["name"]
        assert np.all(hit.sum(axis=0) == m) and np.all(hit.sum(axis=1) == 1), c["name"]


def test_state_concatenates_cases():
    k = [P.index_of("cscl_2x1x1"), P.index_of("one_atom")]
    nat, types, frac, lat = P.state(k)
    assert nat == [4, 1] and types.shape == (5,) and frac.shape == (5, 3) and lat.shape == (2, 3, 3)
    assert frac.dtype == np.float32 and lat.dtype == np.float32 and types.dtype == np.int64
    assert S.MARGIN == P.MARGIN


def test_primitive_validates_on_the_host():
    from chemeleon_amd import Primitive
    from chemeleon_amd.primitive import PrimitiveReport
    p = Primitive()
    assert (p.symprec, p.angle_tolerance) == (0.1, 10.0) and "symprec=0.1" in repr(p)
    assert Primitive(symprec=1, angle_tolerance=30).symprec == 1.0
    for kw in (dict(symprec=0), dict(symprec=-0.1), dict(symprec=1.5), dict(symprec=float("nan")), dict(symprec="0.1"),
               dict(symprec=True), dict(angle_tolerance=0), dict(angle_tolerance=30.5), dict(angle_tolerance=None)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Primitive(**kw)
    rec = np.zeros((2, 16), dtype=np.int32)
    rec[0, :11] = [2, 4, 4, 1, 0, 2, 0, 2, 2, 2, 4]
    rec[0, 11] = np.float32(0.05).view(np.int32)
    rec[0, 12] = 6
    rec[1, :11] = [3, 0, 0, 0, 8, 1, 0, 0, 1, 0, 1]
    rec[1, 12] = -1
    rep = PrimitiveReport(rec.view(np.uint8), [8, 3])
    assert rep.reduced.tolist() == [True, False] and rep.valid.tolist() == [True, False] and len(rep) == 2
    r = rep.record(0)
    assert r["n_prim"] == 2 and r["n_trans"] == 4 and r["hnf"] == ((2, 0, 2), (0, 2, 2), (0, 0, 4)) and r["reduced"]
    assert r["tol"] == float(np.float32(0.05)) and r["lattice_system"] == "cubic" and r["halvings"] == 1
    assert rep.record(1)["failed"] == ["thin"] and rep.record(1)["lattice_system"] is None
