"""Dedup on the device (csrc/dedup.hip, chm_dedup_*, chemeleon_amd.dedup) against the plain restatements of
tests/dedup_cases.py: fingerprints against float64, determinism, invariance, grouping by the leader rule, graph
capture, the argument checks, the torch op and Chemeleon.sample(dedup=...).

Error gate of a fingerprint: e = |F_dev - F_64| / |F_64| <= 16 x the largest e of the float32 numpy restatement
over the same cases (dedup_cases.error_gate; tests/test_dedup_cases.py asserts that it is <= tol / 8). The grouping
cases meet the margin condition asserted there (same-composition distances outside [tol / 2, 2 tol]), so group
and count must equal the plain leader rule over the float64 distances exactly. The non-transitive chain is built
from fingerprints passed directly (distances 0.04, 0.04, 0.08): no fingerprint rounding is involved, and fp32
rounding of a distance (1e-6) is far from the 20 % between those and tol."""

import numpy as np
import pytest
import torch

from chemeleon_amd import Dedup, Fingerprints, Screen, _lib, dedup_states, fingerprint_states, group_fingerprints
from chemeleon_amd.config import default_config
from chemeleon_amd.dedup import DedupPlan
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from tests import dedup_cases as C

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def to_device(cs):
    nat, a, x, lat = C.batch_arrays(cs)
    return nat, torch.from_numpy(a).to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(lat).to(DEV)


@pytest.fixture(scope="module")
def ragged():
    """The fingerprint cases as one ragged batch on the device and its fingerprints (computed once)."""
    nat, a, x, lat = to_device(C.fingerprint_cases())
    fps = fingerprint_states(nat, a, x, lat)
    return nat, a, x, lat, fps


# ------------------------------------------------------------------------------------------ fingerprints
def test_fingerprints_match_float64(ragged):
    _, _, _, _, fps = ragged
    F64, counts, flags = C.fingerprint_reference()
    F = fps.fp.cpu().numpy()
    assert F.shape == (len(F64), 2 * C.BINS) and F.dtype == np.float32
    np.testing.assert_array_equal(fps.flags.cpu().numpy(), flags)
    np.testing.assert_array_equal(fps.counts.cpu().numpy(), counts)  # (the integer reference, exactly)
    gate, base = C.error_gate(), C.baseline_errors()
    errs = {}
    for g, c in enumerate(C.fingerprint_cases()):
        if flags[g]:
            assert np.all(F[g] == 0), c["name"]
            continue
        errs[c["name"]] = C.rel_error(F[g], F64[g])
        print(f"{c['name']}: device {errs[c['name']]:.3e}, float32 restatement {base[c['name']]:.3e}, gate {gate:.3e}")
    assert max(errs.values()) <= gate, errs
    by = [c["name"] for c in C.fingerprint_cases()]
    assert np.all(F[by.index("all_class_0")][C.BINS:] == 0)


def test_two_runs_and_a_crystal_alone_give_the_same_bits(ragged):
    nat, a, x, lat, fps = ragged
    again = fingerprint_states(nat, a, x, lat)
    F = fps.fp.cpu().numpy()
    np.testing.assert_array_equal(again.fp.cpu().numpy().view(np.uint32), F.view(np.uint32))
    off = np.concatenate([[0], np.cumsum(nat)])
    for g, n in enumerate(nat):
        one = fingerprint_states([n], a[off[g]:off[g + 1]].clone(), x[off[g]:off[g + 1]].clone(),
                                 lat[g:g + 1].clone())
        np.testing.assert_array_equal(one.fp.cpu().numpy().view(np.uint32)[0], F[g].view(np.uint32), err_msg=str(g))
        assert int(one.flags[0]) == int(fps.flags[g])


def test_other_bin_counts_take_the_other_ownership_paths():
    """bins = 8 (16 threads per bin), 24 (a part of the block idle), 200 (two bins per thread)."""
    cs = [c for c in C.fingerprint_cases() if c["name"] in ("n2", "n65", "thin_R3")]
    nat, a, x, lat = to_device(cs)
    for K in (8, 24, 200):
        F = fingerprint_states(nat, a, x, lat, Dedup(bins=K)).fp.cpu().numpy()
        dev, base = [], []
        for g, c in enumerate(cs):
            L, f = c["lattice"].astype(np.float32), c["frac"].astype(np.float32)
            F64 = C.fingerprint_f64(L, f, c["types"], K=K)
            dev.append(C.rel_error(F[g], F64))
            base.append(C.rel_error(C.fingerprint_f32(L, f, c["types"], K=K), F64))
            print(f"K={K} {c['name']}: device {dev[-1]:.3e}, float32 restatement {base[-1]:.3e}")
        assert max(dev) <= 16 * max(base), (K, dev, base)


# ------------------------------------------------------------------------------------------ invariance
def test_transformed_copies_join_their_original_and_moved_copies_do_not():
    for orig, same, moved in C.invariance_cases():
        cs = [orig] + same + moved
        nat, a, x, lat = to_device(cs)
        assert len(set(nat)) >= 3  # (ragged: the supercells)
        rep = dedup_states(nat, a, x, lat)
        k = 1 + len(same)
        assert rep.group[:k].tolist() == [0] * k, (orig["name"], rep.group)
        assert rep.group[k:].tolist() == list(range(k, len(cs)))
        assert rep.count[0] == k and rep.n_groups == 1 + len(moved)


# ------------------------------------------------------------------------------------------ grouping
@pytest.mark.parametrize("B", C.GROUP_SIZES)
def test_groups_equal_the_leader_rule_over_float64_distances(B):
    cs, _ = C.planted(B)
    _, _, _, _, group, count = C.planted_reference(B)
    nat, a, x, lat = to_device(cs)
    rep = dedup_states(nat, a, x, lat)
    np.testing.assert_array_equal(rep.group, group)
    np.testing.assert_array_equal(rep.count, count)
    assert rep.n_groups == int((count > 0).sum()) and not rep.flags.any()


def test_a_list_of_fingerprints_groups_as_the_concatenated_batch():
    cs, _ = C.planted(65)
    _, _, _, _, group, count = C.planted_reference(65)
    whole = to_device(cs)
    first, second = to_device(cs[:40]), to_device(cs[40:])
    fps = [fingerprint_states(*first), fingerprint_states(*second)]
    rep = group_fingerprints(fps)
    one = group_fingerprints(fingerprint_states(*whole))
    np.testing.assert_array_equal(rep.group, one.group)
    np.testing.assert_array_equal(rep.count, one.count)
    np.testing.assert_array_equal(rep.group, group)
    np.testing.assert_array_equal(rep.count, count)


def direct(F, counts=None, flags=None):
    F = np.asarray(F, dtype=np.float32)
    B = len(F)
    counts = np.tile(C.reduced_counts(C.TIO2), (B, 1)) if counts is None else counts
    flags = np.zeros(B, dtype=np.int32) if flags is None else np.asarray(flags, dtype=np.int32)
    return Fingerprints(torch.from_numpy(F).to(DEV), torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(DEV),
                        torch.from_numpy(flags).to(DEV))


def test_non_transitive_chain_follows_the_leader_rule():
    rng = np.random.default_rng(5)
    v = rng.random(2 * C.BINS) + 1.0
    u = rng.standard_normal(2 * C.BINS)
    u -= u.dot(v) / v.dot(v) * v
    u *= 0.04 * np.linalg.norm(v) / np.linalg.norm(u)
    F = np.stack([v, v + u, v + 2 * u])
    D = C.distance_matrix(F.astype(np.float32))
    assert D[0, 1] < 0.045 and D[1, 2] < 0.045 and D[0, 2] > 0.075
    rep = group_fingerprints(direct(F))
    assert rep.group.tolist() == [0, 0, 2] and rep.count.tolist() == [2, 0, 1]
    rep = group_fingerprints(direct(F[[1, 0, 2]]))  # the middle one first: it leads both
    assert rep.group.tolist() == [0, 0, 0] and rep.count.tolist() == [3, 0, 0]


def test_excluded_and_flagged_crystals_are_never_grouped(ragged):
    F = np.tile(np.linspace(1, 2, 2 * C.BINS), (5, 1))
    rep = group_fingerprints(direct(F), exclude=[True, False, False, True, False])
    assert rep.group.tolist() == [-1, 1, 1, -1, 1] and rep.count.tolist() == [0, 3, 0, 0, 0]
    assert rep.representative.tolist() == [False, True, False, False, False]
    rep = group_fingerprints(direct(F, flags=[0, C.DEGENERATE, 0, C.NONFINITE, 0]),
                             exclude=torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8, device=DEV))
    assert rep.group.tolist() == [0, -1, -1, -1, 0] and rep.count.tolist() == [2, 0, 0, 0, 0]
    assert rep.flags.tolist() == [0, C.DEGENERATE, 0, C.NONFINITE, 0]
    # the flagged crystals of the ragged batch (all-zero fingerprints, two of equal composition)
    nat, a, x, lat, fps = ragged
    rep = group_fingerprints(fps)
    for g in np.flatnonzero(rep.flags):
        assert rep.group[g] == -1 and rep.count[g] == 0
    assert np.all(rep.group[rep.flags == 0] >= 0)


def test_swapped_elements_and_other_compositions_are_not_grouped():
    cs = C.swapped_elements()
    nat, a, x, lat = to_device(cs)
    fps = fingerprint_states(nat, a, x, lat)
    F = fps.fp.cpu().numpy()
    np.testing.assert_allclose(F[0][:C.BINS], F[1][:C.BINS], rtol=1e-5, atol=1e-5)  # (equal geometry)
    rep = group_fingerprints(fps, Dedup(tol=0.05))
    assert rep.group.tolist() == [0, 1, 2]
    # even at a tolerance that swallows the distance, another composition stays apart
    rep = group_fingerprints(fps, Dedup(tol=0.5))
    assert rep.group.tolist() == [0, 0, 2]


# ------------------------------------------------------------------------------------------ the C entry points
def run_raw(plan, a, x, lat, fp, counts, flags, group, count, ws, K=C.BINS, tol=C.TOL, **n):
    """chm_dedup_fingerprint then chm_dedup_group with every count overridable -> (rc1, rc2)."""
    lib, B = _lib.load(), len(plan.natoms)
    st = _lib.stream_handle()
    rc1 = lib.chm_dedup_fingerprint(plan.handle, _lib.ptr(a), a.numel(), _lib.ptr(x), x.numel(), _lib.ptr(lat),
                                    lat.numel(), K, C.R_CUT, C.SIGMA, _lib.ptr(fp), n.get("n_fp", fp.numel()),
                                    _lib.ptr(counts), n.get("n_counts", counts.numel()), _lib.ptr(flags),
                                    n.get("n_flags", flags.numel()), st)
    if rc1 != 0 or n.get("only_fingerprint"):
        return rc1, None
    rc2 = lib.chm_dedup_group(B, K, _lib.ptr(fp), fp.numel(), _lib.ptr(counts), counts.numel(), _lib.ptr(flags),
                              flags.numel(), None, 0, tol, _lib.ptr(group), n.get("n_group", group.numel()),
                              _lib.ptr(count), n.get("n_count", count.numel()), _lib.ptr(ws),
                              n.get("ws_bytes", ws.numel()), st)
    return rc1, rc2


def buffers(B, fill=0):
    i32 = dict(dtype=torch.int32, device=DEV)
    return (torch.full((B, 2 * C.BINS), float(fill), device=DEV), torch.full((B, 104), fill, **i32),
            torch.full((B,), fill, **i32), torch.full((B,), fill, **i32), torch.full((B,), fill, **i32),
            torch.zeros(_lib.load().chm_dedup_workspace_bytes(B), dtype=torch.uint8, device=DEV))


def test_graph_replay_equals_eager():
    cs, _ = C.planted(33)
    _, _, _, _, group, count = C.planted_reference(33)
    nat, a, x, lat = to_device(cs)
    plan = DedupPlan(nat, DEV)
    eager = buffers(33)
    assert run_raw(plan, a, x, lat, *eager) == (0, 0), _lib.load().chm_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eager[3].cpu().numpy(), group)
    np.testing.assert_array_equal(eager[4].cpu().numpy(), count)
    out = buffers(33)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert run_raw(plan, a, x, lat, *out) == (0, 0)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in out[:5]:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k in range(5):
            assert torch.equal(out[k], eager[k]), k


def test_run_calls_refuse_mis_sized_buffers():
    cs, _ = C.planted(33)
    nat, a, x, lat = to_device(cs)
    plan = DedupPlan(nat, DEV)
    lib = _lib.load()
    buf = buffers(33, fill=-7)
    need = buf[5].numel()
    for kw, name in [({"n_fp": 33 * 128 - 128}, b"fp"), ({"n_counts": 33 * 104 + 104}, b"counts"),
                     ({"n_flags": 32}, b"flags")]:
        rc, _ = run_raw(plan, a, x, lat, *buf, **kw)
        assert rc == -1 and name in lib.chm_last_error(), (kw, lib.chm_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in buf[:5])  # nothing was enqueued
    fps = fingerprint_states(nat, a, x, lat)
    buf[0].copy_(fps.fp), buf[1].copy_(fps.counts), buf[2].copy_(fps.flags)
    st = _lib.stream_handle()

    def group(**n):
        return lib.chm_dedup_group(33, C.BINS, _lib.ptr(buf[0]), n.get("n_fp", buf[0].numel()), _lib.ptr(buf[1]),
                                   n.get("n_counts", buf[1].numel()), _lib.ptr(buf[2]), buf[2].numel(), None, 0, C.TOL,
                                   _lib.ptr(buf[3]), n.get("n_group", 33), _lib.ptr(buf[4]), n.get("n_count", 33),
                                   _lib.ptr(buf[5]), n.get("ws_bytes", need), st)

    for kw, name in [({"n_fp": 33 * 128 + 1}, b"fp"), ({"n_counts": 33 * 104 - 1}, b"counts"), ({"n_group": 32}, b"group"),
                     ({"n_count": 34}, b"count"), ({"ws_bytes": need - 4}, b"workspace")]:
        assert group(**kw) == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    torch.cuda.synchronize()
    assert bool((buf[3] == -7).all()) and bool((buf[4] == -7).all())  # nothing was enqueued
    assert group() == 0, lib.chm_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf[3].cpu().numpy(), C.planted_reference(33)[4])


# ------------------------------------------------------------------------------------------ torch op, sample()
def test_torch_op_equals_dedup_states():
    from chemeleon_amd import ops
    chem = ops.load()
    cs, _ = C.planted(65)
    nat, a, x, lat = to_device(cs)
    ex = np.zeros(65, dtype=bool)
    ex[[0, 7, 40]] = True
    for exclude in (None, ex):
        rep = dedup_states(nat, a, x, lat, Dedup(), exclude)
        group, count, fp = chem.dedup(a, x, lat, nat, None if exclude is None else torch.from_numpy(exclude).to(DEV),
                                      C.TOL, C.R_CUT, C.SIGMA, C.BINS)
        assert group.dtype == torch.int32 and count.dtype == torch.int32 and fp.shape == (65, 2 * C.BINS)
        np.testing.assert_array_equal(group.cpu().numpy(), rep.group)
        np.testing.assert_array_equal(count.cpu().numpy(), rep.count)
        assert torch.equal(fp, fingerprint_states(nat, a, x, lat).fp)
    with pytest.raises(RuntimeError, match="shape"):
        chem.dedup(a[:-1], x, lat, nat, None, C.TOL, C.R_CUT, C.SIGMA, C.BINS)
    with pytest.raises(RuntimeError, match="bins"):
        chem.dedup(a, x, lat, nat, None, C.TOL, C.R_CUT, C.SIGMA, 4)
    with pytest.raises(RuntimeError, match="tol"):
        chem.dedup(a, x, lat, nat, None, 0.0, C.R_CUT, C.SIGMA, C.BINS)
    with pytest.raises(RuntimeError, match="HIP device only"):
        chem.dedup(a, x, lat.cpu(), nat, None, C.TOL, C.R_CUT, C.SIGMA, C.BINS)


@pytest.fixture(scope="module")
def model100():
    from chemeleon_amd import Chemeleon
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    return m.to(DEV).eval()


def test_sample_returns_the_representatives(model100):
    from chemeleon_amd import screen_states
    cond, null = synthetic_text_embeds(512)
    kw = dict(noise="philox", seed=4, text_embeds=cond, null_text_embeds=null)
    natoms = [6] * 8
    last = None
    for last in model100.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw):
        pass
    _, a, x, lat = last
    a, x, lat = a.clone(), x.clone(), lat.clone()
    # a tolerance so wide that equal compositions group, so that both outcomes occur whatever the samples are
    dd = Dedup(tol=1e6)
    want = dedup_states(natoms, a, x, lat, dd)
    atoms = model100.sample(None, 6, 8, dedup=dd, **kw)
    rep = model100.last_dedup
    np.testing.assert_array_equal(rep.group, want.group)
    np.testing.assert_array_equal(rep.count, want.count)
    keep = np.flatnonzero(rep.representative).tolist()
    assert len(atoms) == rep.n_groups == len(keep) >= 1
    assert [at.info["dedup"]["index"] for at in atoms] == keep
    from chemeleon_amd.modules.schema import step_to_atoms
    every = step_to_atoms(a, x, lat, natoms)
    for at, g in zip(atoms, keep):
        assert at.info["dedup"] == {"index": g, "group": g, "multiplicity": int(rep.count[g])}
        np.testing.assert_array_equal(np.asarray(at.numbers), np.asarray(every[g].numbers))
        np.testing.assert_array_equal(at.get_scaled_positions(), every[g].get_scaled_positions())
    assert sum(at.info["dedup"]["multiplicity"] for at in atoms) == int((rep.group >= 0).sum())
    # with a screen as well: its failures are excluded, never returned and never representatives
    free = screen_states(natoms, a, x, lat, Screen(max_length=1e6, min_distance=1e-6))
    d = float(np.median(free.dmin))
    scr = Screen(max_length=1e6, min_distance=d)
    atoms = model100.sample(None, 6, 8, dedup=Dedup(), screen=scr, **kw)
    rep, srep = model100.last_dedup, model100.last_screen
    assert 0 < srep.valid.sum() < 8
    assert np.all(rep.group[~srep.valid] == -1) and np.all(rep.group[srep.valid] >= 0)
    assert len(atoms) == rep.n_groups and all(srep.valid[at.info["dedup"]["index"]] for at in atoms)
    assert all(at.info["screen"]["valid"] for at in atoms)
    np.testing.assert_array_equal(rep.group, dedup_states(natoms, a, x, lat, Dedup(), ~srep.valid).group)


def test_stream_with_dedup_raises(model100):
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, stream=True, dedup=Dedup())
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, return_trajectory=True, dedup=Dedup())
