"""Structure matching on the device (chemeleon_amd.match, csrc/match.hip) against the float64 restatement of
tests/match_cases.py: matched, flags and the counts exactly; rms, max_dist and scale within a gate of 16 times the
float32 restatement's own largest error against float64 over the same cases (measured on the CPU: rms 4.8e-8,
max_dist 7.0e-7 A, scale 0, so the gate is 1.1e-5, below 1e-3 stol = 3e-4); the winner and the pairing; identical
bytes run to run, alone and in a batch, eager and replayed from a graph; the argument checks; the Python and torch-op
layers; and sample(match=...) / finish_atoms with the other legs.

The cases keep a margin of match_cases.MARGIN between every decision and its bound in float64
(tests/test_match_cases.py), so the float32 arithmetic decides nothing differently from the definition."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import (Cell, Dedup, Match, MatchReport, Reference, Screen, Symmetry, _lib, dedup_states, match_states,
                           screen_states)
from chemeleon_amd.cell import CellPlan
from chemeleon_amd.config import default_config
from chemeleon_amd.match import RECORD_BYTES, MatchPlan
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from tests import match_cases as M

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def on_device(structs):
    nat, types, frac, lat = M.packed(structs)
    return nat, torch.from_numpy(types).to(DEV), torch.from_numpy(frac).to(DEV), torch.from_numpy(lat).to(DEV)


def cell_records(nat, lat):
    rec = torch.zeros(len(nat) * 128, dtype=torch.uint8, device=DEV)
    plan = CellPlan(nat, DEV)  # (kept in a name: the handle must outlive the call)
    rc = _lib.load().chm_cell_run(plan.handle, _lib.ptr(lat), lat.numel(), None, 0, 0.1, 10.0, _lib.ptr(rec), rec.numel(),
                                  _lib.stream_handle())
    assert rc == 0, _lib.load().chm_last_error()
    torch.cuda.synchronize()
    return rec


@pytest.fixture(scope="module")
def refs():
    """The references on the device: (natoms, types, frac, lattices, cell records)."""
    nat, a, x, lat = on_device([s for _, s in M.references()])
    return nat, a, x, lat, cell_records(nat, lat)


def run_raw(state, refs, ref_of, perm=True, out=None, perm_out=None, cell_rec=None, plan=None, **n):
    """chm_match_run with every count overridable -> (rc, out, perm)."""
    nat, a, x, lat = state
    rnat, ra, rx, rlat, rrec = refs
    if cell_rec is None:
        cell_rec = cell_records(nat, lat)
    if out is None:
        out = torch.full((len(nat) * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    if perm and perm_out is None:
        perm_out = torch.full((sum(nat),), -7, dtype=torch.int32, device=DEV)
    plan = plan or MatchPlan(nat, rnat, ref_of, DEV)
    rc = _lib.load().chm_match_run(
        plan.handle, _lib.ptr(cell_rec), n.get("n_rec", cell_rec.numel()), _lib.ptr(a), n.get("n_a", a.numel()),
        _lib.ptr(x), n.get("n_x", x.numel()), _lib.ptr(lat), n.get("n_l", lat.numel()), _lib.ptr(rrec),
        n.get("n_rrec", rrec.numel()), _lib.ptr(ra), n.get("n_ra", ra.numel()), _lib.ptr(rx), n.get("n_rx", rx.numel()),
        _lib.ptr(rlat), n.get("n_rl", rlat.numel()), n.get("ltol", M.LTOL), n.get("stol", M.STOL),
        n.get("angle_tol", M.ANGLE_TOL), _lib.ptr(out), n.get("n_o", out.numel()), _lib.ptr(perm_out),
        n.get("n_p", 0 if perm_out is None else perm_out.numel()), _lib.stream_handle())
    return rc, out, perm_out


@pytest.fixture(scope="module")
def everything(refs):
    """All cases in one batch with their mixed ref_of: (state, ref_of, records [B,64], perm [N]), run once."""
    state = on_device([c["sample"] for c in M.cases()])
    ref_of = [c["ref"] for c in M.cases()]
    rc, out, perm = run_raw(state, refs, ref_of)
    assert rc == 0, _lib.load().chm_last_error()
    return state, ref_of, out.cpu().numpy().reshape(-1, RECORD_BYTES), perm.cpu().numpy()


@pytest.fixture(scope="module")
def gate():
    g = 16 * M.float32_error()
    assert g < 1e-3 * M.STOL
    return g


def test_records_against_the_float64_restatement(everything, gate):
    _, _, records, _ = everything
    rep = MatchReport(records)
    worst = dict.fromkeys(M.FLOAT_FIELDS + ("l",), 0.0)
    for g, (c, want) in enumerate(zip(M.cases(), M.reference("float64"))):
        got = rep.record(g)
        for f in M.INT_FIELDS:
            assert int(got[f]) == int(want[f]), (c["name"], f, got, {q: want[q] for q in M.INT_FIELDS})
        assert got["matched"] == bool(c["matched"]) and got["flags"] == c["flags"], c["name"]
        for f in worst:
            worst[f] = max(worst[f], abs(got[f] - want[f]))
            assert abs(got[f] - want[f]) <= gate, (c["name"], f, got[f], want[f])
        assert not records[g, 48:].any(), c["name"]
        if not want["matched"]:
            assert (got["mapping"], got["anchor"], got["rms"], got["max_dist"]) == (-1, -1, 0.0, 0.0), c["name"]
            continue
        rms = sorted(v[2] for v in want["counting"])
        if len(rms) == 1 or rms[1] - rms[0] > gate:
            assert (got["mapping"], got["anchor"]) == (want["mapping"], want["anchor"]), c["name"]
        else:
            near = {(v[0], v[1]) for v in want["counting"] if v[2] <= rms[0] + gate}
            assert (got["mapping"], got["anchor"]) in near, c["name"]
    print("device error against float64:", worst, "gate", gate, "largest n_mappings", int(rep.n_mappings.max()))
    assert rep.n_matched == sum(c["matched"] for c in M.cases())
    assert rep.match_rate == rep.n_matched / len(rep) and 0 < rep.rms_mean < M.STOL
    assert np.array_equal(rep.mismatch, ~rep.matched)


def test_perm_is_the_winners_pairing(everything, gate):
    _, _, records, perm = everything
    rep = MatchReport(records, perm)
    refs = M.references()
    n0 = 0
    for g, (c, want) in enumerate(zip(M.cases(), M.reference("float64"))):
        n = len(c["sample"]["types"])
        pm = rep.perm[n0:n0 + n]
        n0 += n
        if not rep.matched[g]:
            assert np.all(pm == -1), c["name"]
            continue
        assert sorted(pm.tolist()) == list(range(n)), c["name"]
        assert np.array_equal(c["sample"]["types"][pm], refs[c["ref"]][1]["types"]), c["name"]
        Mw = np.array([(int(rep.mapping[g]) // 3 ** q) % 3 - 1 for q in range(9)]).reshape(3, 3)
        Minv = np.round(np.linalg.inv(Mw.astype(np.float64))).astype(np.int64)
        t = M._mapped(want["xs"], Minv, np.float64)[rep.anchor[g]] - want["xr"][want["p"]]
        rms, maxd = M.score(want["xs"], want["xr"], want["Lr"], want["sL"], Mw, t, pm, want["l"])
        assert abs(rms - rep.rms[g]) <= gate and abs(maxd - rep.max_dist[g]) <= gate, (c["name"], rms, rep.rms[g])


def test_bytes_do_not_depend_on_the_run_or_the_batch(everything, refs):
    state, ref_of, records, perm = everything
    rc, again, perm2 = run_raw(state, refs, ref_of)
    assert rc == 0
    np.testing.assert_array_equal(again.cpu().numpy().reshape(-1, RECORD_BYTES), records)
    np.testing.assert_array_equal(perm2.cpu().numpy(), perm)
    n0 = 0
    for g, c in enumerate(M.cases()):  # B = 1: every case alone, against the same list of references
        n = len(c["sample"]["types"])
        rc, out, pm = run_raw(on_device([c["sample"]]), refs, [c["ref"]])
        assert rc == 0
        np.testing.assert_array_equal(out.cpu().numpy(), records[g], err_msg=c["name"])
        np.testing.assert_array_equal(pm.cpu().numpy(), perm[n0:n0 + n], err_msg=c["name"])
        n0 += n


def test_three_references_and_a_mixed_ref_of(everything):
    _, _, records, _ = everything
    names = ["rutile", "cscl", "quartz"]
    by_name = dict(M.references())
    ref = Reference.from_arrays(*M.packed([by_name[n] for n in names]))
    at = {M.references()[k][0]: k for k in range(len(M.references()))}
    pick = [g for g, c in enumerate(M.cases()) if c["ref"] in [at[n] for n in names]][::2] + \
           [g for g, c in enumerate(M.cases()) if c["name"] == "no_reference"]
    ref_of = [-1 if M.cases()[g]["ref"] < 0 else names.index(M.references()[M.cases()[g]["ref"]][0]) for g in pick]
    assert len(set(ref_of)) == 4
    nat, a, x, lat = on_device([M.cases()[g]["sample"] for g in pick])
    rep = match_states(nat, a, x, lat, Match(ref, ref_of=ref_of))
    want = records[pick].copy()
    want.view(np.int32)[:, 11] = ref_of  # (the record names the reference by its index in the list it was given)
    np.testing.assert_array_equal(rep.records, want)


def test_graph_replay_and_eager_are_byte_identical(refs):
    pick = [g for g, c in enumerate(M.cases()) if len(c["sample"]["types"]) <= 8][::5]
    state = on_device([M.cases()[g]["sample"] for g in pick])
    ref_of = [M.cases()[g]["ref"] for g in pick]
    nat, a, x, lat = state
    plan = MatchPlan(nat, refs[0], ref_of, DEV)
    cell_rec = cell_records(nat, lat)
    rc, eager, eager_perm = run_raw(state, refs, ref_of, plan=plan, cell_rec=cell_rec)
    assert rc == 0
    out, perm = torch.zeros_like(eager), torch.zeros_like(eager_perm)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc, _, _ = run_raw(state, refs, ref_of, out=out, perm_out=perm, plan=plan, cell_rec=cell_rec)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(0x5C)
        perm.fill_(-9)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(perm, eager_perm)


def test_run_refuses_bad_arguments(refs):
    lib = _lib.load()
    pick = [0, 8, 20]
    state = on_device([M.cases()[g]["sample"] for g in pick])
    ref_of = [M.cases()[g]["ref"] for g in pick]
    nat = state[0]
    B, N = len(nat), sum(nat)
    plan = MatchPlan(nat, refs[0], ref_of, DEV)
    cell_rec = cell_records(nat, state[3])
    rc, good, good_perm = run_raw(state, refs, ref_of, plan=plan, cell_rec=cell_rec)
    assert rc == 0
    out = torch.full((B * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    perm = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    for kw, name in [({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"), ({"n_l": 9 * B - 9}, b"lattices"),
                     ({"n_rec": 128 * B - 128}, b"cell records"), ({"n_rrec": 128}, b"ref cell records"),
                     ({"n_ra": 1}, b"ref_atom_types"), ({"n_rx": 3}, b"ref_frac"), ({"n_rl": 9}, b"ref_lattices"),
                     ({"n_o": 64 * B - 64}, b"out"), ({"n_p": N - 1}, b"perm"), ({"ltol": 0.0}, b"ltol"),
                     ({"ltol": 1.5}, b"ltol"), ({"stol": 0.0}, b"stol"), ({"stol": float("nan")}, b"stol"),
                     ({"angle_tol": 30.5}, b"angle_tol"), ({"angle_tol": 0.0}, b"angle_tol")]:
        rc, _, _ = run_raw(state, refs, ref_of, out=out, perm_out=perm, plan=plan, cell_rec=cell_rec, **kw)
        assert rc == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    assert lib.chm_match_run(None, *([None, 0] * 8), 0.2, 0.3, 5.0, None, 0, None, 0, None) == -1
    assert b"plan" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((perm == -7).all())  # nothing was enqueued
    rc, out, perm = run_raw(state, refs, ref_of, out=out, perm_out=perm, plan=plan, cell_rec=cell_rec)
    assert rc == 0 and torch.equal(out, good) and torch.equal(perm, good_perm)
    h = _lib.c_void_p()
    big, one, of = (ctypes.c_int32 * 2)(4, 257), (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 2)(0, 0)
    assert lib.chm_match_create(big, 2, one, 1, of, ctypes.byref(h)) == -3 and b"256" in lib.chm_last_error()
    assert lib.chm_match_create(one, 1, big, 2, of, ctypes.byref(h)) == -3 and b"256" in lib.chm_last_error()
    bad_of = (ctypes.c_int32 * 1)(1)
    assert lib.chm_match_create(one, 1, one, 1, bad_of, ctypes.byref(h)) == -1 and b"ref_of" in lib.chm_last_error()


def test_python_and_torch_op_return_the_ctypes_bytes(everything, refs):
    from chemeleon_amd import ops as ops_module
    chem = ops_module.load()
    (nat, a, x, lat), ref_of, records, perm = everything
    ref = Reference.from_arrays(*M.packed([s for _, s in M.references()]))
    rep = match_states(nat, a, x, lat, Match(ref, ref_of=ref_of), perm=True)
    np.testing.assert_array_equal(rep.records, records)
    np.testing.assert_array_equal(rep.perm, perm)
    assert match_states(nat, a, x, lat, Match(ref, ref_of=ref_of)).perm is None
    rec, pm = chem.match(a, x, lat, nat, refs[1], refs[2], refs[3], refs[0], ref_of, M.LTOL, M.STOL, M.ANGLE_TOL, True)
    assert rec.shape == (len(nat), 64) and rec.dtype == torch.uint8 and pm.dtype == torch.int32
    np.testing.assert_array_equal(rec.cpu().numpy(), records)
    np.testing.assert_array_equal(pm.cpu().numpy(), perm)
    rec, pm = chem.match(a, x, lat, nat, refs[1], refs[2], refs[3], refs[0], ref_of, M.LTOL, M.STOL, M.ANGLE_TOL, False)
    assert pm.shape == (0,)
    np.testing.assert_array_equal(rec.cpu().numpy(), records)
    with pytest.raises(RuntimeError, match="shape"):
        chem.match(a, x[:-1], lat, nat, refs[1], refs[2], refs[3], refs[0], ref_of, 0.2, 0.3, 5.0, False)
    with pytest.raises(RuntimeError, match="ltol"):
        chem.match(a, x, lat, nat, refs[1], refs[2], refs[3], refs[0], ref_of, 0.0, 0.3, 5.0, False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        match_states(nat, a, x.cpu(), lat, Match(ref, ref_of=ref_of))


# --------------------------------------------------------------------------- Chemeleon.sample(match=...)
@pytest.fixture(scope="module")
def model100():
    from chemeleon_amd import Chemeleon
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def final(model100):
    """(kw, natoms, a, x, lat, every structure): the final state of the unconstrained 4 x 6 run, computed once."""
    from chemeleon_amd.modules.schema import step_to_atoms
    cond, null = synthetic_text_embeds(512)
    kw = dict(noise="philox", seed=4, text_embeds=cond, null_text_embeds=null)
    natoms = [6] * 4
    last = None
    for last in model100.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw):
        pass
    _, a, x, lat = last
    a, x, lat = a.clone(), x.clone(), lat.clone()
    return kw, natoms, a, x, lat, step_to_atoms(a, x, lat, natoms)


def same_structure(at, other):
    np.testing.assert_array_equal(np.asarray(at.numbers), np.asarray(other.numbers))
    np.testing.assert_array_equal(at.get_scaled_positions(), other.get_scaled_positions())
    np.testing.assert_array_equal(np.asarray(at.cell), np.asarray(other.cell))


def test_sample_returns_the_matched_crystals(model100, final):
    kw, natoms, a, x, lat, every = final
    ref = Reference.from_arrays([6], a[:6].cpu().numpy(), x[:6].cpu().numpy(), lat[:1].cpu().numpy())
    free = match_states(natoms, a, x, lat, Match(ref))
    assert free.matched[0] and free.rms[0] < 1e-5  # crystal 0 against itself: rounding level
    atoms = model100.sample(None, 6, 4, match=Match(ref, require=True), **kw)
    np.testing.assert_array_equal(model100.last_match.records, free.records)
    keep = np.flatnonzero(free.matched).tolist()
    assert 0 in keep and [at.info["match"]["index"] for at in atoms] == keep
    for at, g in zip(atoms, keep):
        same_structure(at, every[g])
        assert at.info["match"]["matched"] and at.info["match"]["rms"] == float(free.rms[g])
    atoms = model100.sample(None, 6, 4, match=Match(ref), **kw)  # without require the leg only reports
    assert [at.info["match"]["index"] for at in atoms] == [0, 1, 2, 3]
    from_atoms = Reference.from_atoms(every[0])
    again = match_states(natoms, a, x, lat, Match(from_atoms))
    assert again.matched[0] and again.rms[0] < 1e-5
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, stream=True, match=Match(ref))
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, return_trajectory=True, match=Match(ref))
    with pytest.raises(ValueError, match="chemeleon_amd.Match"):
        model100.sample(None, 6, 2, match=ref)
    with pytest.raises(ValueError, match="lists 3 crystals"):
        model100.sample(None, 6, 4, match=Match(ref, ref_of=[0, 0, 0]), **kw)


def test_without_the_keyword_nothing_changes(model100, final):
    from chemeleon_amd import match as match_module
    kw, natoms, a, x, lat, every = final
    plans = len(match_module._plans)
    model100.last_match = None
    atoms = model100.sample(None, 6, 4, **kw)
    assert model100.last_match is None and len(match_module._plans) == plans
    assert len(atoms) == 4
    for at, other in zip(atoms, every):
        same_structure(at, other)  # (bit for bit the state of sample_states on the same seed)
        assert "match" not in (getattr(at, "info", None) or {})


def test_finish_atoms_excludes_the_unmatched_from_the_grouping(final):
    from chemeleon_amd.finish import finish_atoms
    kw, natoms, a, x, lat, every = final
    ref = Reference.from_arrays([6, 6], a[:12].cpu().numpy(), x[:12].cpu().numpy(), lat[:2].cpu().numpy())
    match = Match(ref, ref_of=[0, 0, 1, -1], require=True)  # crystal 0 and 2 against crystal 0 and 1, 3 has none
    free = match_states(natoms, a, x, lat, match)
    assert free.matched[0] and not free.matched[3] and free.flags[3] == M.NO_REFERENCE
    screen = Screen(max_length=1e6, min_distance=1e-6)
    atoms, reports = finish_atoms(natoms, a, x, lat, screen=screen, cell=Cell(), symmetry=Symmetry(), match=match,
                                  dedup=Dedup())
    assert set(reports) == {"screen", "cell", "symmetry", "match", "dedup"}
    np.testing.assert_array_equal(reports["match"].records, free.records)
    failed = ~screen_states(natoms, a, x, lat, screen).valid | free.mismatch
    want = dedup_states(natoms, a, x, lat, Dedup(), failed)
    np.testing.assert_array_equal(reports["dedup"].group, want.group)
    assert np.all(reports["dedup"].group[free.mismatch] == -1) and reports["dedup"].group[0] >= 0
    keep = np.flatnonzero(want.representative).tolist()
    assert [at.info["match"]["index"] for at in atoms] == keep and 0 in keep
    for at, g in zip(atoms, keep):
        same_structure(at, every[g])
        assert at.info["match"]["matched"] and at.info["dedup"]["index"] == g
