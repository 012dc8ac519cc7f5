"""Dedup without a GPU: the float64 reference's invariances, the conditions the shared fixtures
(tests/dedup_cases.py) must keep for the GPU tests to mean what they say (the margin condition, the error gate),
the leader rule on hand-made matrices, Dedup's and group_fingerprints' validation, and the argument checks of
chm_dedup_* that run before the device is touched."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import Dedup, DedupReport, Fingerprints, _lib, dedup_states, fingerprint_states, group_fingerprints
from tests import dedup_cases as C


def f64(c):
    return C.fingerprint_f64(c["lattice"], c["frac"], c["types"])


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("kind", list(C.TRANSFORMS))
def test_reference_is_invariant_under_each_transformation(kind):
    for k, types in enumerate([C.TIO2, [C.SR, C.TI, C.O, C.O, C.O], [C.TI] * 4 + [C.O] * 8]):
        orig = C.random_crystal(40 + k, types)
        copy = C.TRANSFORMS[kind](orig, np.random.default_rng(50 + k))
        if kind in ("2x1x1", "1x2x2"):
            assert len(copy["types"]) == len(types) * (2 if kind == "2x1x1" else 4)
        if kind == "perm":
            assert not np.array_equal(copy["frac"], orig["frac"])
        assert C.distance(f64(orig), f64(copy)) <= 1e-10, (kind, k)


def test_reference_is_invariant_under_combinations_and_not_under_a_moved_atom():
    for orig, same, moved in C.invariance_cases():
        F = f64(orig)
        assert np.linalg.norm(F) > 1
        for c in same:
            assert C.distance(F, f64(c)) <= 1e-10, c["name"]
        for c in moved:
            assert C.distance(F, f64(c)) > C.TOL, c["name"]


def test_a_moved_atom_is_above_the_default_tolerance_without_choosing_seeds():
    for k in range(6):
        orig = C.random_crystal(900 + k, C.TIO2)
        assert C.distance(f64(orig), f64(C.perturbed(orig, 950 + k))) > C.TOL


def test_reference_support_and_taper():
    """One pair at distance d: the bins further than 6 sigma are exactly zero, the nearest bin holds
    2 / n * taper * exp(...), and at r_cut the taper leaves nothing."""
    for d in (1.0, 3.3, C.R_CUT - 5e-5):
        F = C.fingerprint_f64(np.eye(3) * 30.0, [[0.1, 0.1, 0.1], [0.1 + d / 30.0, 0.1, 0.1]], [C.TI, C.O])
        rk = (np.arange(C.BINS) + 0.5) * C.R_CUT / C.BINS
        far = np.abs(rk - d) > C.SUPPORT * C.SIGMA
        assert np.all(F[:C.BINS][far] == 0) and np.all(F[C.BINS:][far] == 0)
        k = int(np.argmin(np.abs(rk - d)))
        want = 0.5 * (1 + np.cos(np.pi * d / C.R_CUT)) * np.exp(-(d - rk[k]) ** 2 / (2 * C.SIGMA ** 2))
        assert F[k] == pytest.approx(want, rel=1e-9, abs=1e-15)
        assert F[C.BINS + k] == pytest.approx(want * 22 * 8 / 15.0 ** 2, rel=1e-9, abs=1e-15)
    assert np.abs(F).max() < 1e-9  # (the last d: 5e-5 A inside r_cut)


# ------------------------------------------------------------------------------------------ the fixtures
def test_fingerprint_cases_cover_the_kernel_boundaries():
    cs = C.fingerprint_cases()
    nat = [len(c["types"]) for c in cs]
    for n in (1, 2, 63, 64, 65, C.TILE - 1, C.TILE, C.TILE + 1):
        assert n in nat
    by = {c["name"]: g for g, c in enumerate(cs)}
    _, counts, flags = C.fingerprint_reference()
    bound = lambda name: C.image_bounds(cs[by[name]]["lattice"].astype(np.float32))[0]  # noqa: E731
    assert int(bound("thin_R3").max()) == 3 and int(bound("thin_R8").max()) == C.MAX_RANGE
    assert bound("beyond_cap").max() > C.MAX_RANGE + 2
    for name, fl in (("beyond_cap", C.DEGENERATE), ("zero_volume", C.DEGENERATE), ("nan_coordinate", C.NONFINITE)):
        assert flags[by[name]] == fl, name
    assert sum(f != 0 for f in flags) == 3
    # no range sits at the cap's threshold, where float32 could decide the flag differently
    for c in cs:
        r = bound(c["name"])
        assert np.all(~np.isfinite(r) | (np.abs(r - (C.MAX_RANGE + 1)) > 0.05)), c["name"]
    assert counts[by["class_outside"]][0] == 2 and counts[by["class_outside"]].sum() == 4  # (104 and -3 are X)
    # the wrapped pair is 8e-6 A apart, not 4 A; the taper pair is 5e-5 A inside r_cut
    w = cs[by["wrap"]]
    assert abs((w["frac"][1, 0] - w["frac"][0, 0] - 1.0) * 4.0) < 1e-5
    t = cs[by["taper"]]
    assert 0 < C.R_CUT - (t["frac"][1, 0] - t["frac"][0, 0]) * 20.0 < 1e-4


def test_channel_1_of_an_all_x_crystal_is_zero_and_flagged_fingerprints_are_zero():
    cs = C.fingerprint_cases()
    F, _, flags = C.fingerprint_reference()
    g = [c["name"] for c in cs].index("all_class_0")
    assert np.all(F[g][C.BINS:] == 0) and np.linalg.norm(F[g][:C.BINS]) > 1
    assert np.all(F[flags != 0] == 0)


def test_error_gate_is_far_inside_the_tolerance():
    """The float32 restatement's own error sets the gate (16 x its largest), and the gate is at most tol / 8:
    fingerprint rounding is no part of a grouping decision."""
    errs = C.baseline_errors()
    assert len(errs) == len(C.fingerprint_cases()) - 3
    for name, e in errs.items():
        print(f"{name}: float32 restatement {e:.3e}")
    assert 0 < C.error_gate() <= C.TOL / 8


@pytest.mark.parametrize("B", C.GROUP_SIZES)
def test_margin_condition_of_the_planted_batches(B):
    """Every same-composition pair's float64 distance lies outside [tol / 2, 2 tol]."""
    cs, labels = C.planted(B)
    assert len(cs) == B
    F, counts, flags, D, group, count = C.planted_reference(B)
    assert not flags.any()
    for g in range(B):
        for h in range(g + 1, B):
            if np.array_equal(counts[g], counts[h]):
                assert not (C.TOL / 2 <= D[g, h] <= 2 * C.TOL), (g, h, D[g, h])
                assert (D[g, h] <= C.TOL) == (labels[g] == labels[h]), (g, h, D[g, h])
    # with such margins the leader rule finds the planted membership
    for g in range(B):
        assert labels[group[g]] == labels[g]
    assert count.sum() == B and (count > 0).sum() == len(set(labels))
    if B >= 33:
        assert len({len(c["types"]) for c in cs}) >= 3 and count.max() >= 3  # (ragged natoms: supercells)


def test_margin_condition_of_the_invariance_and_element_cases():
    for orig, same, moved in C.invariance_cases():
        F = [f64(dict(c, lattice=c["lattice"].astype(np.float32), frac=c["frac"].astype(np.float32)))
             for c in [orig] + same + moved]
        D = C.distance_matrix(np.stack(F))
        iu = np.triu_indices(len(F), 1)
        assert not np.any((D[iu] >= C.TOL / 2) & (D[iu] <= 2 * C.TOL))
    F, counts, _ = C.reference(C.swapped_elements())
    D = C.distance_matrix(F)
    assert np.array_equal(counts[0], counts[1]) and not np.array_equal(counts[0], counts[2])
    assert D[0, 1] > 2 * C.TOL                                   # same composition: channel 1 tells them apart
    assert C.distance(F[0][:C.BINS], F[1][:C.BINS]) < 1e-12      # channel 0 does not
    assert C.distance(F[0][:C.BINS], F[2][:C.BINS]) < 1e-12      # equal geometry, another composition


# ------------------------------------------------------------------------------------------ the leader rule
def test_leader_rule_on_hand_made_matrices():
    def sym(B, pairs):
        M = np.zeros((B, B), dtype=bool)
        for g, h in pairs:
            M[g, h] = M[h, g] = True
        return M

    # a non-transitive chain A~B, B~C, not A~C: B joins A, C is a representative of its own
    g, c = C.leader(sym(3, [(0, 1), (1, 2)]))
    assert g.tolist() == [0, 0, 2] and c.tolist() == [2, 0, 1]
    # C matches both representatives A and B (which do not match): it joins the earliest
    g, c = C.leader(sym(3, [(0, 2), (1, 2)]))
    assert g.tolist() == [0, 1, 0] and c.tolist() == [2, 1, 0]
    # a member (1) is no representative: 2 matches only 1 and stays alone
    g, c = C.leader(sym(4, [(0, 1), (1, 2), (0, 3)]))
    assert g.tolist() == [0, 0, 2, 0] and c.tolist() == [3, 0, 1, 0]
    # excluded crystals get -1 and lead nothing
    g, c = C.leader(sym(3, [(0, 1), (0, 2), (1, 2)]), ok=[False, True, True])
    assert g.tolist() == [-1, 1, 1] and c.tolist() == [0, 2, 0]
    g, c = C.leader(sym(1, []))
    assert g.tolist() == [0] and c.tolist() == [1]


# ------------------------------------------------------------------------------------------ the Python layer
def test_dedup_defaults():
    d = Dedup()
    assert (d.tol, d.r_cut, d.sigma, d.bins) == (C.TOL, C.R_CUT, C.SIGMA, C.BINS)
    assert "tol=0.05" in repr(d)


@pytest.mark.parametrize("kw", [dict(tol=0.0), dict(tol=-0.1), dict(tol=float("nan")), dict(tol=float("inf")),
                                dict(r_cut=0.0), dict(r_cut=float("inf")), dict(sigma=0.0), dict(sigma=-1.0),
                                dict(sigma=float("nan")), dict(bins=7), dict(bins=257), dict(bins=64.0),
                                dict(bins=True), dict(tol="0.05")])
def test_dedup_refuses_bad_arguments(kw):
    with pytest.raises(ValueError):
        Dedup(**kw)


def test_report_fields():
    r = DedupReport([0, 0, 2, -1], [2, 0, 1, 0], [0, 0, 0, 8])
    assert r.representative.tolist() == [True, False, True, False] and r.n_groups == 2 and len(r) == 4
    assert r.record(2) == {"index": 2, "group": 2, "multiplicity": 1}


def test_bad_input_is_refused_before_a_device_is_touched():
    a, x, lat = torch.zeros(5, dtype=torch.long), torch.zeros(5, 3), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="shapes"):
        fingerprint_states([2, 2], a, x, lat)
    with pytest.raises(ValueError, match="Dedup"):
        fingerprint_states([2, 3], a, x, lat, dedup=0.05)
    with pytest.raises(ValueError, match="natoms"):
        fingerprint_states([], a, x, lat)
    with pytest.raises(RuntimeError, match="HIP device only"):
        fingerprint_states([2, 3], a, x, lat)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dedup_states([2, 3], a, x, lat)
    fp = Fingerprints(torch.zeros(3, 128), torch.zeros(3, 104, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="Fingerprints"):
        group_fingerprints([])
    with pytest.raises(ValueError, match="Fingerprints"):
        group_fingerprints([fp, "x"])
    with pytest.raises(ValueError, match="bins"):
        group_fingerprints(fp, Dedup(bins=32))
    with pytest.raises(ValueError, match="exclude"):
        group_fingerprints(fp, exclude=[True, False])
    with pytest.raises(ValueError, match="exclude"):
        group_fingerprints(fp, exclude=np.zeros(3))
    with pytest.raises(ValueError, match="counts"):
        group_fingerprints(Fingerprints(fp.fp, fp.counts[:2], fp.flags))
    with pytest.raises(ValueError, match="float32"):
        group_fingerprints(Fingerprints(fp.fp.double(), fp.counts, fp.flags))
    with pytest.raises(RuntimeError, match="HIP device only"):
        group_fingerprints(fp)


def test_sample_refuses_dedup_with_streaming():
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    cfg = default_config()
    cfg["timesteps"] = 10
    m = Chemeleon(cfg)
    for kw in (dict(stream=True), dict(return_trajectory=True)):
        with pytest.raises(ValueError, match="finished structures"):
            m.sample(None, 4, 2, dedup=Dedup(), **kw)
    with pytest.raises(ValueError, match="Dedup"):
        m.sample(None, 4, 2, dedup=0.05)


# ------------------------------------------------------------------------------------------ C entry points
def test_entry_points_refuse_null_and_bad_arguments_without_gpu():
    lib = _lib.load()
    out = ctypes.c_void_p()
    nat = (ctypes.c_int32 * 3)(1, 5, 70)
    assert lib.chm_dedup_create(None, 3, ctypes.byref(out)) == -1 and b"natoms" in lib.chm_last_error()
    assert lib.chm_dedup_create(nat, 0, ctypes.byref(out)) == -1 and b"num_graphs" in lib.chm_last_error()
    assert lib.chm_dedup_create(nat, 3, None) == -1 and b"out" in lib.chm_last_error()
    bad = (ctypes.c_int32 * 3)(1, 0, 70)
    assert lib.chm_dedup_create(bad, 3, ctypes.byref(out)) == -1 and b"natoms[1]" in lib.chm_last_error()
    assert not out.value
    x = ctypes.c_void_p(0x10000)  # (never dereferenced: every call below is refused before any HIP call)
    assert lib.chm_dedup_fingerprint(None, x, 1, x, 3, x, 9, 64, 6.0, 0.15, x, 128, x, 104, x, 1, None) == -1
    assert b"plan" in lib.chm_last_error()
    for K, r_cut, sigma, name in [(7, 6.0, 0.15, b"K "), (257, 6.0, 0.15, b"K "), (64, 0.0, 0.15, b"r_cut"),
                                  (64, float("inf"), 0.15, b"r_cut"), (64, 6.0, -0.1, b"sigma"),
                                  (64, 6.0, float("nan"), b"sigma")]:
        assert lib.chm_dedup_fingerprint(None, x, 1, x, 3, x, 9, K, r_cut, sigma, x, 128, x, 104, x, 1, None) == -1
        assert name in lib.chm_last_error(), (K, r_cut, sigma, lib.chm_last_error())
    lib.chm_dedup_destroy(None)
    assert lib.chm_dedup_workspace_bytes(0) == 0 and lib.chm_dedup_workspace_bytes(-3) == 0
    assert lib.chm_dedup_workspace_bytes(1) >= 8 and lib.chm_dedup_workspace_bytes(33) >= 33 * 2 * 4 + 33 * 4
    need = lib.chm_dedup_workspace_bytes(3)

    def group(B=3, K=64, fp=x, n_fp=384, counts=x, n_counts=312, flags=x, n_flags=3, ex=None, n_ex=0, tol=0.05,
              grp=x, n_grp=3, cnt=x, n_cnt=3, ws=x, ws_bytes=need):
        return lib.chm_dedup_group(B, K, fp, n_fp, counts, n_counts, flags, n_flags, ex, n_ex, tol, grp, n_grp, cnt,
                                   n_cnt, ws, ws_bytes, None)

    for kw, name in [(dict(B=0), b"B must"), (dict(B=-1), b"B must"), (dict(K=7), b"K "), (dict(K=257), b"K "),
                     (dict(tol=0.0), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(tol=float("inf")), b"tol"),
                     (dict(fp=None), b"fp"), (dict(n_fp=383), b"fp"), (dict(counts=None), b"counts"),
                     (dict(n_counts=104), b"counts"), (dict(n_flags=2), b"flags"), (dict(flags=None), b"flags"),
                     (dict(ex=x, n_ex=2), b"exclude"), (dict(n_ex=3), b"exclude"), (dict(grp=None), b"group"),
                     (dict(n_grp=4), b"group"), (dict(cnt=None), b"count"), (dict(n_cnt=2), b"count"),
                     (dict(ws=None), b"workspace"), (dict(ws_bytes=need - 1), b"workspace")]:
        assert group(**kw) == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
