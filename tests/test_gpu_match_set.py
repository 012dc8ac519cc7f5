"""The reference-set search on the device (chemeleon_amd.match_set, csrc/match.hip: chm_match_set_*) against its
definition restated in numpy over the float64 restatement of tests/match_cases.py (tests/match_set_cases.py): the key
bit for bit; known, ref, n_candidates, n_matched, flags and every launched pair's matched and flags exactly; rms and
max_dist of every pair and every winner within 16 times the float32 restatement's own largest error against float64
over the same pairs (measured on the CPU, tests/test_match_set_cases.py: 7.0e-7, so the gate is 1.1e-5, below 1e-3
stol = 3e-4); the winner's record equal to match_states' for that sample against that one reference, byte for byte;
a sample's record the same bytes alone, in another batch, run to run and with the set in another original order; a
captured graph replayed on a state of other compositions equal to an eager run on it; the exclusion mask; the
argument checks; the torch op; and finish_atoms(screen=, search=, dedup=MatchDedup())."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import (Match, MatchDedup, MatchSet, MatchSetReport, Reference, ReferenceSet, Screen, _lib,
                           match_group_states, match_set_states, match_states, screen_states)
from chemeleon_amd.cell import CellPlan
from chemeleon_amd.match_set import MatchSetPlan
from tests import match_cases as M
from tests import match_set_cases as S

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def on_device(names):
    nat, types, frac, lat = M.packed([S.structures()[c] for c in names])
    return nat, torch.from_numpy(types).to(DEV), torch.from_numpy(frac).to(DEV), torch.from_numpy(lat).to(DEV)


@pytest.fixture(scope="module")
def refset():
    return ReferenceSet.from_arrays(*S.packed_set())


@pytest.fixture(scope="module")
def reports(refset):
    """name -> (state, MatchSetReport) of every batch, each run once through match_set_states."""
    out = {}
    for b, (names, mask) in S.batches().items():
        state = on_device(names)
        out[b] = (state, match_set_states(*state, MatchSet(refset), mask))
    return out


@pytest.fixture(scope="module")
def gate():
    g = 16 * S.float32_error()
    assert g < 1e-3 * M.STOL
    return g


def test_records_and_pairs_against_the_float64_restatement(reports, gate):
    names = S.reference_names()
    worst = 0.0
    for b, (state, rep) in reports.items():
        want = S.expected(b)
        assert len(rep) == len(want)
        for g, (s, w) in enumerate(zip(S.batches()[b][0], want)):
            assert int(rep.key[g]) == w["key"], (b, s)
            got = (bool(rep.known[g]), int(rep.ref[g]), int(rep.n_candidates[g]), int(rep.n_matched[g]), int(rep.flags[g]))
            assert got == (w["known"], w["ref"], w["n_candidates"], w["n_matched"], w["flags"]), (b, s, got)
            assert bool(rep.novel[g]) == (not w["known"] and not w["flags"] & (S.EXCLUDED | M.NO_LATTICE))
            assert (w["n_candidates"] == 0 or int(rep.lo[g]) == w["lo"]) and (rep.position[g] >= 0) == w["known"]
            refs, matched, rms = rep.candidates(g)
            assert refs.tolist() == w["cands"], (b, s)
            first = int(rep.first[g])
            for k, r in enumerate(w["records"]):
                assert bool(matched[k]) == bool(r["matched"]) and rep.pair_flags[first + k] == r["flags"], (b, s, names[refs[k]])
                err = max(abs(float(rms[k]) - r["rms"]), abs(float(rep.pair_max_dist[first + k]) - r["max_dist"]))
                print(b, s, names[refs[k]], "matched", r["matched"], "rms", rms[k], "error", err)
                assert err <= gate, (b, s, names[refs[k]], err)
                worst = max(worst, err)
            assert abs(float(rep.rms[g]) - w["rms"]) <= gate and abs(float(rep.max_dist[g]) - w["max_dist"]) <= gate, (b, s)
            if w["known"]:  # the winner's pair record, through its sorted position
                at = first + int(rep.position[g]) - int(rep.lo[g])
                np.testing.assert_array_equal(rep.records[g, :12], rep.pair_records[at, :12])
                assert rep.pair_ref[at] == w["ref"] and rep.pair_sample[at] == g
            else:
                assert not rep.records[g, :8].any() and rep.ref[g] == -1
            assert rep.record(g)["known"] == w["known"] and rep.record(g)["ref"] == w["ref"]
        assert rep.first.tolist() == np.concatenate([[0], np.cumsum(rep.n_candidates)[:-1]]).tolist()
        assert rep.n_known == sum(w["known"] for w in want) and len(rep.pair_records) == rep.n_candidates.sum()
    print("largest device error against float64:", worst, "gate", gate)
    rep = reports["first65"][1]
    assert rep.novelty_rate == rep.n_novel / (len(rep) - 1) and not rep.mismatch.any()  # (one sample has no reduced cell)


def test_the_winner_equals_match_states_against_that_reference(reports, refset):
    (nat, a, x, lat), rep = reports["first65"]
    ref = Reference.from_arrays(*S.packed_set())
    single = match_states(nat, a, x, lat, Match(ref, ref_of=rep.ref.tolist()))
    known = np.flatnonzero(rep.known)
    assert len(known) > 30 and single.matched[known].all() and not single.matched[~rep.known].any()
    np.testing.assert_array_equal(rep.records[known, :8], single.records[known, :8])  # rms, max_dist
    np.testing.assert_array_equal(rep.flags[known], single.flags[known])


def test_bytes_do_not_depend_on_the_run_the_batch_or_the_order_of_the_set(reports, refset):
    names, _ = S.batches()["first65"]
    state, rep = reports["first65"]
    again = match_set_states(*state, MatchSet(refset))
    np.testing.assert_array_equal(again.records, rep.records)
    np.testing.assert_array_equal(again.pair_records, rep.pair_records)
    # every sample alone ... (the ones that decide something; a batch of one each)
    for g in (3, 17, 40):
        alone = match_set_states(*on_device([names[g]]), MatchSet(refset))
        np.testing.assert_array_equal(alone.records[0, :40], rep.records[g, :40])
        np.testing.assert_array_equal(alone.candidates(0)[2], rep.candidates(g)[2])
    # ... at other places of another batch ...
    moved = list(range(40, 65)) + list(range(3, 40, 2))
    other = match_set_states(*on_device([names[g] for g in moved]), MatchSet(refset))
    np.testing.assert_array_equal(other.records[:, :40], rep.records[moved, :40])
    for k, g in enumerate(moved):
        a, b = int(other.first[k]), int(rep.first[g])
        np.testing.assert_array_equal(other.pair_records[a:a + other.n_candidates[k]], rep.pair_records[b:b + rep.n_candidates[g]])
    # ... and with the set given in another order: the same structures win, under their new indices
    set_names = S.reference_names()
    perm = np.random.default_rng(11).permutation(len(set_names))
    new_names = tuple(set_names[k] for k in perm)
    new_of = {int(old): new for new, old in enumerate(perm)}
    shuffled = match_set_states(*state, MatchSet(ReferenceSet.from_arrays(*S.packed_set(new_names))))
    twins = [set_names.index(t) for t in S.TWINS]
    for g in range(len(rep)):
        np.testing.assert_array_equal(shuffled.records[g, :16], rep.records[g, :16])
        np.testing.assert_array_equal(shuffled.records[g, 24:40], rep.records[g, 24:40])
        if rep.ref[g] in twins:
            assert shuffled.ref[g] == min(new_of[t] for t in twins)
        else:
            assert shuffled.ref[g] == (new_of[int(rep.ref[g])] if rep.known[g] else -1)
    assert sum(rep.ref[g] in twins for g in range(len(rep))) >= 2


def cell_run(plan, lat, rec):
    rc = _lib.load().chm_cell_run(plan.handle, _lib.ptr(lat), lat.numel(), None, 0, 0.1, 10.0, _lib.ptr(rec), rec.numel(),
                                  _lib.stream_handle())
    assert rc == 0, _lib.load().chm_last_error()


def buffers(plan, B, fill=0xAB):
    """(out, pair records, workspace) filled with a pattern."""
    return (torch.full((48 * B,), fill, dtype=torch.uint8, device=DEV),
            torch.full((16 * plan.num_pairs_max,), fill, dtype=torch.uint8, device=DEV),
            torch.full((plan.workspace_bytes,), fill, dtype=torch.uint8, device=DEV))


def run_raw(state, plan, cell_rec, refs, bufs, exclude=None, **n):
    """chm_match_set_run with every count overridable -> rc."""
    nat, a, x, lat = state
    ra, rx, rlat, rrec = refs
    out, prec, ws = bufs
    return _lib.load().chm_match_set_run(
        plan.handle, _lib.ptr(cell_rec), n.get("n_rec", cell_rec.numel()), _lib.ptr(a), n.get("n_a", a.numel()),
        _lib.ptr(x), n.get("n_x", x.numel()), _lib.ptr(lat), n.get("n_l", lat.numel()), _lib.ptr(rrec),
        n.get("n_rrec", rrec.numel()), _lib.ptr(ra), n.get("n_ra", ra.numel()), _lib.ptr(rx), n.get("n_rx", rx.numel()),
        _lib.ptr(rlat), n.get("n_rl", rlat.numel()), _lib.ptr(exclude),
        n.get("n_ex", 0 if exclude is None else exclude.numel()), n.get("ltol", M.LTOL), n.get("stol", M.STOL),
        n.get("angle_tol", M.ANGLE_TOL), _lib.ptr(out), n.get("n_o", out.numel()), _lib.ptr(prec),
        n.get("n_p", prec.numel()), _lib.ptr(ws), n.get("n_ws", ws.numel()), _lib.stream_handle())


def test_a_replayed_graph_follows_the_new_atom_types(refset):
    """Two batches of the same atom counts and other compositions: the graph is captured on the first, the state is
    overwritten in place with the second, and the replay equals an eager run on the second (and the other way)."""
    pool, st = S.pool()[:33], S.structures()
    by_size = {}
    for name in S.pool() + tuple(n for n in S.reference_names() if n.startswith("filler")):
        by_size.setdefault(len(st[name]["types"]), []).append(name)
    # sample g of the second batch: the next structure of its size (cyclic), so most compositions change
    second = [by_size[len(st[s]["types"])][(by_size[len(st[s]["types"])].index(s) + 1) % len(by_size[len(st[s]["types"])])]
              for s in pool]
    one, two = on_device(pool), on_device(second)
    assert one[0] == two[0] and not torch.equal(one[1], two[1])
    nat = one[0]
    B = len(nat)
    want = [match_set_states(*s, MatchSet(refset)) for s in (one, two)]
    assert not np.array_equal(want[0].key, want[1].key) and not np.array_equal(want[0].known, want[1].known)
    assert not np.array_equal(want[0].n_candidates, want[1].n_candidates)  # (so the pair list is laid out anew)
    plan, cells = MatchSetPlan(nat, refset, DEV), CellPlan(nat, DEV)
    refs = refset.on(DEV)
    a, x, lat = (t.clone() for t in one[1:])
    cell_rec = torch.zeros(B * 128, dtype=torch.uint8, device=DEV)
    bufs = buffers(plan, B, 0x11)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            cell_run(cells, lat, cell_rec)
            assert run_raw((nat, a, x, lat), plan, cell_rec, refs, bufs) == 0
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 0, 1):
        for t, src in zip((a, x, lat), (one, two)[k][1:]):
            t.copy_(src)
        bufs[0].fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        got = MatchSetReport(bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), refset.order)
        np.testing.assert_array_equal(got.records, want[k].records)
        np.testing.assert_array_equal(got.pair_records, want[k].pair_records)


def test_the_exclusion_mask(reports):
    (_, free), (_, masked) = reports["first33"], reports["excluded"]
    mask = S.batches()["excluded"][1]
    flat = np.array([not S.usable(s) for s in S.batches()["excluded"][0]])
    assert flat[mask].any() and not flat[mask].all()  # (an excluded sample without a reduced cell carries both flags)
    np.testing.assert_array_equal(masked.flags[mask], S.EXCLUDED | np.where(flat[mask], M.NO_LATTICE, 0))
    assert (masked.n_candidates[mask] == 0).all()
    assert not masked.known[mask].any() and not masked.novel[mask].any() and free.known[mask].any()
    np.testing.assert_array_equal(masked.key, free.key)
    np.testing.assert_array_equal(masked.records[~mask, :40], free.records[~mask, :40])
    for g in np.flatnonzero(~mask):
        np.testing.assert_array_equal(masked.candidates(g)[2], free.candidates(g)[2])


def test_run_refuses_bad_arguments(refset):
    lib = _lib.load()
    names, _ = S.batches()["first33"]
    state = on_device(names)
    nat = state[0]
    B, N, R, NR = len(nat), sum(nat), len(refset), sum(refset.natoms)
    plan, cells = MatchSetPlan(nat, refset, DEV), CellPlan(nat, DEV)
    P = plan.num_pairs_max
    sizes = list(refset.natoms)
    assert P == sum(sizes.count(n) for n in nat) > 0
    refs = refset.on(DEV)
    cell_rec = torch.zeros(B * 128, dtype=torch.uint8, device=DEV)
    cell_run(cells, state[3], cell_rec)
    ex = torch.zeros(B, dtype=torch.uint8, device=DEV)
    good = buffers(plan, B)
    assert run_raw(state, plan, cell_rec, refs, good, ex) == 0
    bufs = buffers(plan, B)
    for kw, name in [({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"), ({"n_l": 9 * B - 9}, b"lattices"),
                     ({"n_rec": 128 * B - 128}, b"cell records"), ({"n_rrec": 128 * R + 128}, b"ref cell records"),
                     ({"n_ra": NR - 1}, b"ref_atom_types"), ({"n_rx": 3 * NR - 3}, b"ref_frac"),
                     ({"n_rl": 9 * R + 9}, b"ref_lattices"), ({"n_ex": B - 1}, b"exclude"), ({"n_o": 48 * B - 48}, b"out"),
                     ({"n_p": 16 * P - 16}, b"pair records"), ({"n_ws": plan.workspace_bytes - 1}, b"workspace"),
                     ({"ltol": 0.0}, b"ltol"), ({"ltol": 1.5}, b"ltol"), ({"stol": 0.0}, b"stol"),
                     ({"stol": float("nan")}, b"stol"), ({"angle_tol": 30.5}, b"angle_tol"), ({"angle_tol": 0.0}, b"angle_tol")]:
        assert run_raw(state, plan, cell_rec, refs, bufs, ex, **kw) == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    assert lib.chm_match_set_run(None, *([None, 0] * 9), 0.2, 0.3, 5.0, *([None, 0] * 3), None) == -1
    assert b"plan" in lib.chm_last_error()
    torch.cuda.synchronize()
    for t in bufs:
        assert bool((t == 0xAB).all())  # nothing was enqueued
    assert run_raw(state, plan, cell_rec, refs, bufs, ex) == 0
    torch.cuda.synchronize()
    used = 16 * int(MatchSetReport(good[0].cpu().numpy(), good[1].cpu().numpy(), refset.order).n_candidates.sum())
    assert torch.equal(bufs[0], good[0]) and torch.equal(bufs[1][:used], good[1][:used])
    assert bool((bufs[1][used:] == 0xAB).all()) and used < 16 * P  # (the list is compact: its tail is left alone)
    # create: sizes, the sort and the permutation
    h = _lib.c_void_p()
    i32, u64 = ctypes.c_int32, ctypes.c_uint64
    assert lib.chm_match_set_create((i32 * 2)(4, 257), 2, (i32 * 1)(4), (u64 * 1)(5), (i32 * 1)(0), 1, ctypes.byref(h)) == -3
    assert b"256" in lib.chm_last_error()
    assert lib.chm_match_set_create((i32 * 1)(4), 1, (i32 * 1)(257), (u64 * 1)(5), (i32 * 1)(0), 1, ctypes.byref(h)) == -3
    assert lib.chm_match_set_create((i32 * 1)(4), 1, (i32 * 2)(4, 3), (u64 * 2)(5, 5), (i32 * 2)(0, 1), 2, ctypes.byref(h)) == -1
    assert b"sorted" in lib.chm_last_error()
    assert lib.chm_match_set_create((i32 * 1)(4), 1, (i32 * 2)(4, 4), (u64 * 2)(6, 5), (i32 * 2)(0, 1), 2, ctypes.byref(h)) == -1
    assert lib.chm_match_set_create((i32 * 1)(4), 1, (i32 * 2)(4, 4), (u64 * 2)(5, 5), (i32 * 2)(1, 0), 2, ctypes.byref(h)) == -1
    assert lib.chm_match_set_create((i32 * 1)(4), 1, (i32 * 2)(4, 4), (u64 * 2)(5, 5), (i32 * 2)(0, 0), 2, ctypes.byref(h)) == -1
    assert b"permutation" in lib.chm_last_error()
    assert lib.chm_match_set_create((i32 * 1)(0), 1, (i32 * 1)(4), (u64 * 1)(5), (i32 * 1)(0), 1, ctypes.byref(h)) == -1
    assert lib.chm_match_set_num_pairs_max(None) == 0 and lib.chm_match_set_workspace_bytes(None) == 0
    with pytest.raises(RuntimeError, match="HIP device only"):
        match_set_states(nat, state[1], state[2].cpu(), state[3], MatchSet(refset))
    with pytest.raises(ValueError, match="require"):
        MatchSet(refset, require=True)
    with pytest.raises(ValueError, match="stol"):
        MatchSet(refset, stol=0.0)
    with pytest.raises(ValueError, match="ReferenceSet"):
        MatchSet(Reference.from_arrays(*S.packed_set()))
    # a batch with no candidate at all: no pair list, and everything is novel
    lone = on_device(["p1_three"])
    assert MatchSetPlan(lone[0], refset, DEV).num_pairs_max == 0
    rep = match_set_states(*lone, MatchSet(refset))
    assert rep.novel.tolist() == [True] and len(rep.pair_records) == 0


def test_torch_op_returns_the_ctypes_bytes(reports, refset):
    from chemeleon_amd import ops as ops_module
    chem = ops_module.load()
    ra, rx, rlat, _ = refset.on(DEV)
    lists = (list(refset.natoms), refset.keys.view(np.int64).tolist(), refset.order.tolist())
    for b in ("first33", "excluded", "first1"):
        (nat, a, x, lat), rep = reports[b]
        mask = S.batches()[b][1]
        ex = None if mask is None else torch.from_numpy(mask).to(DEV)
        rec, pairs = chem.match_set(a, x, lat, nat, ra, rx, rlat, *lists, ex, M.LTOL, M.STOL, M.ANGLE_TOL)
        assert rec.shape == (len(nat), 48) and rec.dtype == torch.uint8 and pairs.shape[1] == 16
        np.testing.assert_array_equal(rec.cpu().numpy(), rep.records)
        np.testing.assert_array_equal(pairs.cpu().numpy()[:len(rep.pair_records)], rep.pair_records)
        assert not pairs.cpu().numpy()[len(rep.pair_records):].any()
    (nat, a, x, lat), _ = reports["first33"]
    with pytest.raises(RuntimeError, match="shape"):
        chem.match_set(a, x[:-1], lat, nat, ra, rx, rlat, *lists, None, 0.2, 0.3, 5.0)
    with pytest.raises(RuntimeError, match="ltol"):
        chem.match_set(a, x, lat, nat, ra, rx, rlat, *lists, None, 0.0, 0.3, 5.0)
    with pytest.raises(RuntimeError, match="ref_keys"):
        chem.match_set(a, x, lat, nat, ra, rx, rlat, lists[0], lists[1][:-1], lists[2], None, 0.2, 0.3, 5.0)


def test_finish_atoms_returns_the_valid_novel_unique_structures(refset):
    from chemeleon_amd.finish import finish_atoms
    names = [s for s in S.pool()[:33] if S.usable(s)]  # (the zero-volume cell cannot become a structure's cell)
    nat, a, x, lat = on_device(names)
    screen = Screen(max_length=11.0, min_distance=1e-6)  # the 12 A supercells fail
    failed = ~screen_states(nat, a, x, lat, screen).valid
    free = match_set_states(nat, a, x, lat, MatchSet(refset))
    assert failed.any() and not failed.all() and free.known[~failed].any() and free.novel[~failed].any()
    for require, out in (("novel", ~free.novel), ("known", ~free.known)):
        search = MatchSet(refset, require=require)
        atoms, got = finish_atoms(nat, a, x, lat, screen=screen, search=search, dedup=MatchDedup())
        assert set(got) == {"screen", "search", "dedup"} and isinstance(got["search"], MatchSetReport)
        np.testing.assert_array_equal(got["search"].records, free.records)
        np.testing.assert_array_equal(got["search"].mismatch, out)
        want = match_group_states(nat, a, x, lat, MatchDedup(), failed | out)
        np.testing.assert_array_equal(got["dedup"].group, want.group)
        keep = np.flatnonzero(want.representative).tolist()
        assert 0 < len(keep) < (~(failed | out)).sum() + 1 and not (failed | out)[keep].any()
        assert [at.info["dedup"]["index"] for at in atoms] == keep
        for at, g in zip(atoms, keep):
            assert at.info["search"] == dict(free.record(g), index=g) and at.info["search"][require]
            assert at.info["screen"]["index"] == g
    # without the keyword nothing of it runs; only the search: everything comes back, each with its record
    atoms, got = finish_atoms(nat, a, x, lat, screen=screen)
    assert set(got) == {"screen"} and all("search" not in at.info for at in atoms)
    atoms, got = finish_atoms(nat, a, x, lat, search=MatchSet(refset))
    assert len(atoms) == len(nat) and [at.info["search"]["known"] for at in atoms] == free.known.tolist()
