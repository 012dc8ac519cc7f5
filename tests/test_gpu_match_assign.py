"""Pairing by assignment on the device (pairing="assignment" of Match / MatchDedup / MatchSet, csrc/match.hip) against
the float64 restatement of tests/assign_cases.py: matched, flags, the counts and n_assigned exactly; rms, max_dist and
scale within a gate of 16 times the float32 restatement's own largest error against float64 over the same cases (the
rule of tests/test_gpu_match.py; measured on the CPU: rms 5.7e-8, max_dist 7.2e-7 A, scale 0, so the gate is 1.15e-5,
below 1e-3 stol = 3e-4); the pairing where the restatement's is unique, and its float64 cost within the gate of the optimum; every case of
match_cases.cases() unchanged; identical bytes run to run, alone and in a batch, eager and replayed; pairing 0 through
the new entry points = the old entry points; the grouping, the set search and sample(); the refusals."""

import numpy as np
import pytest
import torch

from chemeleon_amd import (Match, MatchDedup, MatchReport, MatchSet, Reference, ReferenceSet, _lib, match_group_states,
                           match_set_states, match_states)
from chemeleon_amd.cell import CellPlan
from chemeleon_amd.config import default_config
from chemeleon_amd.match import RECORD_BYTES, MatchPlan
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from tests import assign_cases as A
from tests import match_cases as M

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
NEAREST, ASSIGNMENT = 0, 1


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


def with_records(structs):
    nat, a, x, lat = on_device(structs)
    return nat, a, x, lat, cell_records(nat, lat)


def run_raw(state, refs, ref_of, pairing=ASSIGNMENT, out=None, perm_out=None, plan=None, old=False, **n):
    """chm_match_run_pairing (or, with old, chm_match_run) with every count overridable -> (rc, out, perm)."""
    nat, a, x, lat, cell_rec = state
    rnat, ra, rx, rlat, rrec = refs
    if out is None:
        out = torch.full((len(nat) * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    if perm_out is None:
        perm_out = torch.full((sum(nat),), -7, dtype=torch.int32, device=DEV)
    plan = plan or MatchPlan(nat, rnat, ref_of, DEV)
    args = [plan.handle, _lib.ptr(cell_rec), cell_rec.numel(), _lib.ptr(a), n.get("n_a", a.numel()), _lib.ptr(x), x.numel(),
            _lib.ptr(lat), lat.numel(), _lib.ptr(rrec), rrec.numel(), _lib.ptr(ra), ra.numel(), _lib.ptr(rx), rx.numel(),
            _lib.ptr(rlat), rlat.numel(), M.LTOL, M.STOL, M.ANGLE_TOL, _lib.ptr(out), n.get("n_o", out.numel()),
            _lib.ptr(perm_out), n.get("n_p", perm_out.numel()), _lib.stream_handle()]
    lib = _lib.load()
    rc = lib.chm_match_run(*args) if old else lib.chm_match_run_pairing(*args, pairing)
    return rc, out, perm_out


@pytest.fixture(scope="module")
def refs():
    return with_records([c["ref"] for c in A.cases()])


@pytest.fixture(scope="module")
def everything(refs):
    """All cases in one batch, case g against reference g: (state, ref_of, records [B,64], perm [N]), run once."""
    state = with_records([c["sample"] for c in A.cases()])
    ref_of = list(range(len(A.cases())))
    rc, out, perm = run_raw(state, refs, ref_of)
    assert rc == 0, _lib.load().chm_last_error()
    return state, ref_of, out.cpu().numpy().reshape(-1, RECORD_BYTES), perm.cpu().numpy()


@pytest.fixture(scope="module")
def gate():
    err = A.float32_error()
    print("float32 restatement against float64:", err)
    assert 16 * err < 1e-3 * M.STOL
    return 16 * err


def test_records_against_the_float64_restatement(everything, gate):
    _, _, records, perm = everything
    rep = MatchReport(records, perm)
    worst, n0 = dict.fromkeys(M.FLOAT_FIELDS + ("l",), 0.0), 0
    for g, (c, want) in enumerate(zip(A.cases(), A.reference("float64"))):
        got, n = rep.record(g), len(c["ref"]["types"])
        pm = rep.perm[n0:n0 + n]
        n0 += n
        print(c["name"], {f: got[f] for f in A.INT_FIELDS}, got["rms"], want["rms"])
        for f in A.INT_FIELDS:
            assert int(got[f]) == int(want[f]), (c["name"], f, got, {q: want[q] for q in A.INT_FIELDS})
        assert got["matched"] == bool(c["matched"]) and got["flags"] == c["flags"], c["name"]
        assert ("many_assignments" in got["failed"]) == bool(c["flags"] & A.MANY_ASSIGNMENTS)
        assert not records[g, 52:].any(), c["name"]
        for f in worst:
            worst[f] = max(worst[f], abs(got[f] - want[f]))
            assert abs(got[f] - want[f]) <= gate, (c["name"], f, got[f], want[f])
        if not want["matched"]:
            assert (got["mapping"], got["anchor"], got["rms"], got["max_dist"]) == (-1, -1, 0.0, 0.0), c["name"]
            assert np.all(pm == -1), c["name"]
            continue
        rms = sorted(v[2] for v in want["counting"])
        clear = len(rms) == 1 or rms[1] - rms[0] > gate
        if clear:
            assert (got["mapping"], got["anchor"]) == (want["mapping"], want["anchor"]), c["name"]
        else:
            assert (got["mapping"], got["anchor"]) in {(v[0], v[1]) for v in want["counting"] if v[2] <= rms[0] + gate}, c["name"]
        # the pairing: a type-preserving bijection whose score is the record's; the restatement's where that is unique
        assert sorted(pm.tolist()) == list(range(n)), c["name"]
        assert np.array_equal(c["sample"]["types"][pm], c["ref"]["types"]), c["name"]
        Mw = np.array([(got["mapping"] // 3 ** q) % 3 - 1 for q in range(9)]).reshape(3, 3)
        Minv = np.round(np.linalg.inv(Mw.astype(np.float64))).astype(np.int64)
        t = M._mapped(want["xs"], Minv, np.float64)[got["anchor"]] - want["xr"][want["p"]]
        score, maxd = M.score(want["xs"], want["xr"], want["Lr"], want["sL"], Mw, t, pm, want["l"])
        assert abs(score - got["rms"]) <= gate and abs(maxd - got["max_dist"]) <= gate, (c["name"], score, got["rms"])
        if clear and want["collided"]:
            assert want["assign_gap"] > M.MARGIN
            assert np.array_equal(pm, want["perm"]), (c["name"], pm, want["perm"])
            # optimality: the float64 cost of the device's pairing against the float64 optimum, in units of c^2
            mine = float(want["cost"][np.arange(n), pm].sum())
            assert (mine - want["assign_cost"]) / want["c2"] <= gate, c["name"]
    print("device error against float64:", worst, "gate", gate)


def test_the_three_atom_cell_matches_only_under_assignment(refs):
    g = next(k for k, c in enumerate(A.cases()) if c["name"] == "three")
    c = A.cases()[g]
    ref = Reference.from_arrays(*M.packed([c["ref"]]))
    nat, a, x, lat = on_device([c["sample"]])
    near = match_states(nat, a, x, lat, Match(ref))
    assert not near.matched[0] and near.n_survivors[0] == 0 and near.n_candidates[0] == 16 and near.n_assigned[0] == 0
    rep = match_states(nat, a, x, lat, Match(ref, pairing="assignment"), perm=True)
    assert rep.matched[0] and abs(rep.rms[0] - 0.077) < 1e-3 and rep.n_assigned[0] == 2
    assert rep.perm.tolist() == [0, 1, 2] and rep.record(0)["n_assigned"] == 2


def test_the_cases_of_the_nearest_rule_are_unchanged():
    structs = [s for _, s in M.references()]
    mrefs = with_records(structs)
    state = with_records([c["sample"] for c in M.cases()])
    ref_of = [c["ref"] for c in M.cases()]
    rc, old, old_perm = run_raw(state, mrefs, ref_of, old=True)
    assert rc == 0
    rc, zero, zero_perm = run_raw(state, mrefs, ref_of, pairing=NEAREST)
    assert rc == 0 and torch.equal(zero, old) and torch.equal(zero_perm, old_perm)   # pairing 0 = the old entry point
    rc, new, new_perm = run_raw(state, mrefs, ref_of, pairing=ASSIGNMENT)
    assert rc == 0
    a, b = MatchReport(old.cpu().numpy()), MatchReport(new.cpu().numpy())
    assert not a.records[:, 48:].any()
    for f in ("matched", "flags", "n_mappings", "n_candidates"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.rms.view(np.int32), b.rms.view(np.int32))            # the winner's rms bits
    assert np.all(b.n_survivors >= a.n_survivors)


def test_bytes_do_not_depend_on_the_run_the_batch_or_a_graph(everything, refs):
    state, ref_of, records, perm = everything
    rc, again, perm2 = run_raw(state, refs, ref_of)
    assert rc == 0
    np.testing.assert_array_equal(again.cpu().numpy().reshape(-1, RECORD_BYTES), records)
    np.testing.assert_array_equal(perm2.cpu().numpy(), perm)
    n0 = 0
    for g, c in enumerate(A.cases()):
        n = len(c["sample"]["types"])
        if n <= 65:  # B = 1: the case alone, against the same list of references
            rc, out, pm = run_raw(with_records([c["sample"]]), refs, [g])
            assert rc == 0
            np.testing.assert_array_equal(out.cpu().numpy(), records[g], err_msg=c["name"])
            np.testing.assert_array_equal(pm.cpu().numpy(), perm[n0:n0 + n], err_msg=c["name"])
        n0 += n
    plan = MatchPlan(state[0], refs[0], ref_of, DEV)
    out, pm = torch.zeros(records.size, dtype=torch.uint8, device=DEV), torch.zeros(len(perm), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc, _, _ = run_raw(state, refs, ref_of, out=out, perm_out=pm, plan=plan)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(0x5C)
        pm.fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().reshape(-1, RECORD_BYTES), records)
        np.testing.assert_array_equal(pm.cpu().numpy(), perm)


def _three_and_others():
    by = {c["name"]: c for c in A.cases()}
    three = by["three"]
    return [three["ref"], by["blocks_of_one"]["ref"], three["sample"], by["chain"]["ref"]]


def test_grouping_merges_the_collided_sample_only_under_assignment():
    structs = _three_and_others()
    nat, a, x, lat = on_device(structs)
    near = match_group_states(nat, a, x, lat, MatchDedup())
    assert near.group.tolist() == [0, 1, 2, 3] and not near.n_assigned.any() and not near.pair_n_assigned.any()
    rep = match_group_states(nat, a, x, lat, MatchDedup(pairing="assignment"))
    assert rep.group.tolist() == [0, 1, 0, 3] and rep.count.tolist() == [2, 1, 0, 1]
    assert rep.matched.tolist() == [False, False, True, False] and rep.flags.tolist() == [0, 0, 0, 0]
    assert rep.n_assigned[2] == 2 and rep.pairs.tolist() == [[0, 2]] and rep.pair_n_assigned.tolist() == [2] and abs(rep.rms[2] - 0.077) < 1e-3
    again = match_group_states(nat, a, x, lat, MatchDedup(pairing="assignment"))
    np.testing.assert_array_equal(again.records, rep.records)
    np.testing.assert_array_equal(again.pair_records, rep.pair_records)


def test_the_set_search_finds_the_collided_sample_only_under_assignment():
    structs = _three_and_others()
    known = ReferenceSet.from_arrays(*M.packed([structs[1], structs[0], structs[3]]))
    nat, a, x, lat = on_device([structs[2], structs[3]])
    near = match_set_states(nat, a, x, lat, MatchSet(known))
    assert near.known.tolist() == [False, True] and near.novel.tolist() == [True, False] and not near.n_assigned.any()
    rep = match_set_states(nat, a, x, lat, MatchSet(known, pairing="assignment"))
    assert rep.known.tolist() == [True, True] and rep.ref.tolist() == [1, 2] and rep.flags.tolist() == [0, 0]
    assert rep.n_assigned[0] == 2 and rep.record(0)["n_assigned"] == 2 and abs(rep.rms[0] - 0.077) < 1e-3
    again = match_set_states(nat, a, x, lat, MatchSet(known, pairing="assignment"))
    np.testing.assert_array_equal(again.records, rep.records)
    np.testing.assert_array_equal(again.pair_records, rep.pair_records)


def test_sample_carries_the_pairing():
    from chemeleon_amd import Chemeleon
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    model = Chemeleon(cfg)
    model.decoder.load_state_dict(synthetic_state_dict(default_config()))
    model = model.to(DEV).eval()
    cond, null = synthetic_text_embeds(512)
    kw = dict(noise="philox", seed=4, text_embeds=cond, null_text_embeds=null)
    three = A.cases()[0]["ref"]
    six = dict(lattice=three["lattice"], types=np.array([11, 11, 17, 17, 17, 17]),
               frac=np.vstack([three["frac"], three["frac"] + 0.31]).astype(np.float32))
    ref = Reference.from_arrays(*M.packed([six]))
    plain = model.sample(None, 6, 4, match=Match(ref), **kw)
    plain_records = model.last_match.records.copy()
    atoms = model.sample(None, 6, 4, match=Match(ref, pairing="assignment"), **kw)
    rep = model.last_match
    assert len(atoms) == len(plain) == 4 and not plain_records[:, 48:].any()
    for k in range(4):  # the same structures; the record names how many candidates were paired by assignment
        assert atoms[k].info["match"]["n_assigned"] == int(rep.n_assigned[k]) and plain[k].info["match"]["n_assigned"] == 0
        assert np.array_equal(atoms[k].get_scaled_positions(), plain[k].get_scaled_positions())
    assert np.array_equal(rep.records[:, 16:32], plain_records[:, 16:32])  # mapping, anchor, n_mappings, n_candidates
    assert not rep.records[:, 52:].any() and np.all((rep.n_assigned >= 0) & (rep.n_assigned <= 64))


def test_run_refuses_bad_arguments(everything, refs):
    state, ref_of, records, _ = everything
    lib = _lib.load()
    plan = MatchPlan(state[0], refs[0], ref_of, DEV)
    B, N = len(state[0]), sum(state[0])
    out = torch.full((B * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    perm = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    for kw, name in [({"pairing": 2}, b"pairing"), ({"pairing": -1}, b"pairing"), ({"n_a": N - 1}, b"atom_types"),
                     ({"n_o": 64 * B - 64}, b"out"), ({"n_p": N - 1}, b"perm")]:
        rc, _, _ = run_raw(state, refs, ref_of, out=out, perm_out=perm, plan=plan, **kw)
        assert rc == -1 and name in lib.chm_last_error(), (kw, lib.chm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((perm == -7).all())  # nothing was enqueued
    assert lib.chm_match_run_pairing(None, *([None, 0] * 8), 0.2, 0.3, 5.0, None, 0, None, 0, None, 7) == -1
    assert lib.chm_match_group_run_pairing(None, *([None, 0] * 5), 0.2, 0.3, 5.0, *([None, 0] * 5), None, 7) == -1
    assert lib.chm_match_set_run_pairing(None, *([None, 0] * 9), 0.2, 0.3, 5.0, *([None, 0] * 3), None, 7) == -1
    assert b"pairing" in lib.chm_last_error()
