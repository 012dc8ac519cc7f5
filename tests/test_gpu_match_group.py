"""Grouping by matching on the device (chemeleon_amd.match_group, csrc/match.hip: chm_match_group_*) against the
float64 restatement of tests/match_cases.py applied to every pair and the plain leader rule
(tests/match_group_cases.py): group and count exactly; matched of every launched pair exactly; rms and max_dist of
every member against its leader within a gate of 16 times the float32 restatement's own largest error against
float64 over the same pairs (measured on the CPU, tests/test_match_group_cases.py: 8.7e-7, so the gate is 1.4e-5,
below 1e-3 stol = 3e-4); each member's record equal to match_states' for that crystal against its leader as a
Reference, byte for byte; identical bytes run to run, in another batch, eager and replayed from a graph; the
argument checks; the torch op; and finish_atoms(dedup=MatchDedup()) behind a screen."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import Match, MatchDedup, Reference, Screen, _lib, match_group_states, match_states, screen_states
from chemeleon_amd.cell import CellPlan
from chemeleon_amd.match_group import EXCLUDED, MatchGroupPlan, MatchGroupReport, pair_table
from tests import match_cases as M
from tests import match_group_cases as G

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def on_device(names):
    nat, types, frac, lat = M.packed([G.crystals()[c] for c in names])
    return nat, torch.from_numpy(types).to(DEV), torch.from_numpy(frac).to(DEV), torch.from_numpy(lat).to(DEV)


def cell_records(nat, lat):
    rec = torch.zeros(len(nat) * 128, dtype=torch.uint8, device=DEV)
    plan = CellPlan(nat, DEV)  # (kept in a name: the handle must outlive the call)
    rc = _lib.load().chm_cell_run(plan.handle, _lib.ptr(lat), lat.numel(), None, 0, 0.1, 10.0, _lib.ptr(rec), rec.numel(),
                                  _lib.stream_handle())
    assert rc == 0, _lib.load().chm_last_error()
    torch.cuda.synchronize()
    return rec


def buffers(plan, B, fill=0xAB):
    """(group, count, out, pair records, workspace) filled with a pattern."""
    return (torch.full((B,), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV),
            torch.full((32 * B,), fill, dtype=torch.uint8, device=DEV),
            torch.full((16 * plan.num_pairs,), fill, dtype=torch.uint8, device=DEV),
            torch.full((plan.workspace_bytes,), fill, dtype=torch.uint8, device=DEV))


def run_raw(state, plan, cell_rec, bufs, exclude=None, **n):
    """chm_match_group_run with every count overridable -> rc."""
    nat, a, x, lat = state
    group, count, out, prec, ws = bufs
    return _lib.load().chm_match_group_run(
        plan.handle, _lib.ptr(cell_rec), n.get("n_rec", cell_rec.numel()), _lib.ptr(a), n.get("n_a", a.numel()),
        _lib.ptr(x), n.get("n_x", x.numel()), _lib.ptr(lat), n.get("n_l", lat.numel()), _lib.ptr(exclude),
        n.get("n_ex", 0 if exclude is None else exclude.numel()), n.get("ltol", M.LTOL), n.get("stol", M.STOL),
        n.get("angle_tol", M.ANGLE_TOL), _lib.ptr(group), n.get("n_g", group.numel()), _lib.ptr(count),
        n.get("n_c", count.numel()), _lib.ptr(out), n.get("n_o", out.numel()), _lib.ptr(prec),
        n.get("n_p", prec.numel()), _lib.ptr(ws), n.get("n_ws", ws.numel()), _lib.stream_handle())


@pytest.fixture(scope="module")
def reports():
    """name -> (state, MatchGroupReport) of every batch, each run once through match_group_states."""
    out = {}
    for b, (names, mask) in G.batches().items():
        state = on_device(names)
        out[b] = (state, match_group_states(*state, MatchDedup(), mask))
    return out


@pytest.fixture(scope="module")
def gate():
    g = 16 * G.float32_error()
    assert g < 1e-3 * M.STOL
    return g


def test_groups_and_pairs_against_the_float64_restatement(reports, gate):
    worst = 0.0
    for b, (state, rep) in reports.items():
        names, mask = G.batches()[b]
        want = G.expected(b)
        assert rep.pairs.tolist() == [list(p) for p in want["pairs"]], b
        np.testing.assert_array_equal(rep.group, want["group"], err_msg=b)
        np.testing.assert_array_equal(rep.count, want["count"], err_msg=b)
        assert rep.n_groups == int((want["count"] > 0).sum())
        np.testing.assert_array_equal(rep.pair_matched, want["matched"], err_msg=b)
        at = {p: k for k, p in enumerate(want["pairs"])}
        for k, ((h, g), r) in enumerate(zip(want["pairs"], want["records"])):
            if r is None:  # an excluded crystal or one without a reduced cell: not searched
                gone = [c for c in (h, g) if mask is not None and mask[c]]
                flat = [c for c in (h, g) if not G.usable(names[c])]
                assert rep.pair_flags[k] == (EXCLUDED if gone else 0) | (M.NO_LATTICE if flat else 0), (b, h, g)
                assert rep.pair_rms[k] == 0 and rep.pair_max_dist[k] == 0
                continue
            assert rep.pair_flags[k] == r["flags"], (b, names[h], names[g])
            err = max(abs(float(rep.pair_rms[k]) - r["rms"]), abs(float(rep.pair_max_dist[k]) - r["max_dist"]))
            print(b, names[h], names[g], "matched", r["matched"], "rms", rep.pair_rms[k], "error", err)
            assert err <= gate, (b, names[h], names[g], err)
            worst = max(worst, err)
        for g in range(len(names)):
            lead = int(rep.group[g])
            if lead < 0:
                gone, flat = mask is not None and mask[g], not G.usable(names[g])
                assert rep.flags[g] == (EXCLUDED if gone else 0) | (M.NO_LATTICE if flat else 0), (b, g)
            if lead < 0 or lead == g:
                assert (rep.rms[g], rep.max_dist[g], rep.matched[g], rep.ref[g], rep.pair[g]) == (0, 0, False, -1, -1)
                assert not rep.records[g, 24:].any() and (lead < 0 or rep.flags[g] == 0)
                continue
            k = at[(lead, g)]
            r = want["records"][k]
            assert rep.ref[g] == lead and rep.pair[g] == k and rep.matched[g] and rep.flags[g] == r["flags"]
            assert abs(float(rep.rms[g]) - r["rms"]) <= gate and abs(float(rep.max_dist[g]) - r["max_dist"]) <= gate, (b, g)
            np.testing.assert_array_equal(rep.records[g, :16], rep.pair_records[k])
            assert rep.record(g) == {"index": g, "group": lead, "multiplicity": 0, "rms": float(rep.rms[g])}
    print("largest device error against float64:", worst, "gate", gate)
    assert reports["first65"][1].n_searched == sum(r is not None and not r["flags"] & ~M.MANY_MAPPINGS
                                                   for r in G.expected("first65")["records"])


def test_members_equal_match_states_against_their_leader(reports):
    for b in ("first65", "excluded", "chain_bac"):
        (nat, a, x, lat), rep = reports[b]
        names, _ = G.batches()[b]
        leaders = [int(r) for r in np.flatnonzero(rep.count > 0)]
        ref = Reference.from_arrays(*M.packed([G.crystals()[names[r]] for r in leaders]))
        ref_of = [leaders.index(int(rep.group[g])) if rep.group[g] >= 0 and rep.group[g] != g else -1
                  for g in range(len(names))]
        single = match_states(nat, a, x, lat, Match(ref, ref_of=ref_of))
        members = np.flatnonzero(np.array(ref_of) >= 0)
        assert len(members) == (rep.group >= 0).sum() - len(leaders) > 0
        np.testing.assert_array_equal(rep.records[members, :8], single.records[members, :8])  # rms, max_dist
        np.testing.assert_array_equal(rep.flags[members], single.flags[members])
        np.testing.assert_array_equal(rep.matched[members], single.matched[members])
        assert single.matched[members].all()


def test_bytes_do_not_depend_on_the_run_or_the_batch(reports):
    names, mask = G.batches()["first65"]
    state, rep = reports["first65"]
    again = match_group_states(*state, MatchDedup(), mask)
    np.testing.assert_array_equal(again.records, rep.records)
    np.testing.assert_array_equal(again.pair_records, rep.pair_records)
    np.testing.assert_array_equal(again.group, rep.group)
    np.testing.assert_array_equal(again.count, rep.count)
    # the same crystals at other places of another batch, among other crystals: a pair's record is the same
    parts = [list(range(40, 65)), list(range(3, 40, 2))]
    moved = parts[0] + parts[1]
    other = match_group_states(*on_device([names[g] for g in moved]), MatchDedup())
    here = {(int(h), int(g)): k for k, (h, g) in enumerate(rep.pairs)}
    same = 0
    for k, (h, g) in enumerate(other.pairs):
        was = (moved[h], moved[g])
        if was in here:  # (the pairs inside each part keep their order; across the parts the roles are exchanged)
            np.testing.assert_array_equal(other.pair_records[k], rep.pair_records[here[was]], err_msg=str(was))
            same += 1
    assert same > 60


def test_graph_replay_and_eager_are_byte_identical():
    names, mask = G.batches()["excluded"]
    state = on_device(names)
    nat = state[0]
    plan = MatchGroupPlan(nat, DEV)
    cell_rec = cell_records(nat, state[3])
    ex = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    eager = buffers(plan, len(nat))
    assert run_raw(state, plan, cell_rec, eager, ex) == 0, _lib.load().chm_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eager[0].cpu().numpy(), G.expected("excluded")["group"])
    bufs = buffers(plan, len(nat), 0x11)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert run_raw(state, plan, cell_rec, bufs, ex) == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in bufs:
            t.fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(bufs[:4], eager[:4]):
            assert torch.equal(got, want)


def test_run_refuses_bad_arguments():
    lib = _lib.load()
    names, _ = G.batches()["first31"]
    state = on_device(names)
    nat = state[0]
    B, N = len(nat), sum(nat)
    plan = MatchGroupPlan(nat, DEV)
    P = plan.num_pairs
    assert P == len(G.pairs_of(names)) == len(pair_table(nat))
    cell_rec = cell_records(nat, state[3])
    ex = torch.zeros(B, dtype=torch.uint8, device=DEV)
    good = buffers(plan, B)
    assert run_raw(state, plan, cell_rec, good, ex) == 0
    bufs = buffers(plan, B)
    for kw, name in [({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"), ({"n_l": 9 * B - 9}, b"lattices"),
                     ({"n_rec": 128 * B - 128}, b"cell records"), ({"n_ex": B - 1}, b"exclude"), ({"n_g": B - 1}, b"group"),
                     ({"n_c": B + 1}, b"count"), ({"n_o": 32 * B - 32}, b"out"), ({"n_p": 16 * P - 16}, b"pair records"),
                     ({"n_ws": plan.workspace_bytes - 1}, b"workspace"), ({"ltol": 0.0}, b"ltol"), ({"ltol": 1.5}, b"ltol"),
                     ({"stol": 0.0}, b"stol"), ({"stol": float("nan")}, b"stol"), ({"angle_tol": 30.5}, b"angle_tol"),
                     ({"angle_tol": 0.0}, b"angle_tol")]:
        assert run_raw(state, plan, cell_rec, bufs, ex, **kw) == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    assert lib.chm_match_group_run(None, *([None, 0] * 5), 0.2, 0.3, 5.0, *([None, 0] * 5), None) == -1
    assert b"plan" in lib.chm_last_error()
    torch.cuda.synchronize()
    for t in bufs[2:]:
        assert bool((t == 0xAB).all())  # nothing was enqueued
    assert bool((bufs[0] == -7).all()) and bool((bufs[1] == -7).all())
    assert run_raw(state, plan, cell_rec, bufs, ex) == 0
    torch.cuda.synchronize()
    for got, want in zip(bufs[:4], good[:4]):
        assert torch.equal(got, want)
    h = _lib.c_void_p()
    big = (ctypes.c_int32 * 2)(4, 257)
    assert lib.chm_match_group_create(big, 2, ctypes.byref(h)) == -3 and b"256" in lib.chm_last_error()
    assert lib.chm_match_group_create((ctypes.c_int32 * 1)(0), 1, ctypes.byref(h)) == -1
    assert lib.chm_match_group_num_pairs(None) == 0 and lib.chm_match_group_workspace_bytes(None) == 0
    with pytest.raises(RuntimeError, match="HIP device only"):
        match_group_states(nat, state[1], state[2].cpu(), state[3])


def test_torch_op_returns_the_ctypes_bytes(reports):
    from chemeleon_amd import ops as ops_module
    chem = ops_module.load()
    for b in ("first33", "excluded", "first1"):
        (nat, a, x, lat), rep = reports[b]
        mask = G.batches()[b][1]
        ex = None if mask is None else torch.from_numpy(mask).to(DEV)
        group, count, rec, pairs = chem.match_group(a, x, lat, nat, ex, M.LTOL, M.STOL, M.ANGLE_TOL)
        assert rec.shape == (len(nat), 32) and rec.dtype == torch.uint8 and group.dtype == torch.int32
        assert pairs.shape == (len(rep.pairs), 16)
        np.testing.assert_array_equal(group.cpu().numpy(), rep.group)
        np.testing.assert_array_equal(count.cpu().numpy(), rep.count)
        np.testing.assert_array_equal(rec.cpu().numpy(), rep.records)
        np.testing.assert_array_equal(pairs.cpu().numpy(), rep.pair_records)
    (nat, a, x, lat), _ = reports["first33"]
    with pytest.raises(RuntimeError, match="shape"):
        chem.match_group(a, x[:-1], lat, nat, None, 0.2, 0.3, 5.0)
    with pytest.raises(RuntimeError, match="ltol"):
        chem.match_group(a, x, lat, nat, None, 0.0, 0.3, 5.0)
    with pytest.raises(RuntimeError, match="exclude"):
        chem.match_group(a, x, lat, nat, torch.zeros(3, dtype=torch.bool, device=DEV), 0.2, 0.3, 5.0)


def test_finish_atoms_returns_the_representatives_behind_a_screen(reports):
    from chemeleon_amd.finish import finish_atoms
    from chemeleon_amd.modules.schema import step_to_atoms
    (nat, a, x, lat), free = reports["first33"]
    names, _ = G.batches()["first33"]
    ok = [g for g in range(len(nat)) if G.usable(names[g])]  # (the zero-volume cell cannot become a structure's cell)
    nat, a, x, lat = on_device([names[g] for g in ok])
    free = match_group_states(nat, a, x, lat)
    screen = Screen(max_length=11.0, min_distance=1e-6)  # the 12 A supercell fails: a representative of the free run
    failed = ~screen_states(nat, a, x, lat, screen).valid
    big = [names[g] for g in ok].index("sc_65")
    assert failed[big] and free.group[big] == big and not failed.all()
    atoms, got = finish_atoms(nat, a, x, lat, screen=screen, dedup=MatchDedup())
    assert set(got) == {"screen", "dedup"} and isinstance(got["dedup"], MatchGroupReport)
    want = match_group_states(nat, a, x, lat, MatchDedup(), failed)
    np.testing.assert_array_equal(got["dedup"].records, want.records)
    np.testing.assert_array_equal(got["dedup"].group, want.group)
    assert (want.group[failed] == -1).all() and (want.flags[failed] == EXCLUDED).all()
    keep = np.flatnonzero(want.representative).tolist()
    assert big not in keep and len(keep) == want.n_groups and 0 < len(keep) < len(nat) - failed.sum()
    assert [at.info["dedup"]["index"] for at in atoms] == keep
    every = step_to_atoms(a, x, lat, nat)
    for at, g in zip(atoms, keep):
        assert at.info["dedup"] == {"index": g, "group": g, "multiplicity": int(want.count[g]), "rms": 0.0}
        assert at.info["screen"]["index"] == g
        np.testing.assert_array_equal(np.asarray(at.numbers), np.asarray(every[g].numbers))
        np.testing.assert_array_equal(np.asarray(at.cell), np.asarray(every[g].cell))
