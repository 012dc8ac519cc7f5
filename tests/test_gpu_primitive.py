"""Primitive cells on the device (chemeleon_amd.primitive, csrc/prim.hip) against the numpy restatements of
tests/prim_cases.py: the records, the lattices, the packed coordinates and types against the float32 restatement
bit for bit, alone and in ragged batches of two orders; the argument checks; stream capture; the Python and
torch-op layers; and the caveats of the symmetry, matching and grouping legs, which primitive= removes.

The cases keep a margin of prim_cases.MARGIN between every distance test and its tolerance in float64
(tests/test_prim_cases.py), so the float32 arithmetic decides nothing differently from the definition."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import (Match, MatchDedup, Primitive, Reference, Symmetry, _lib, match_group_states, match_states,
                           primitive_states, symmetry_states)
from chemeleon_amd import match as match_module
from chemeleon_amd.cell import CellPlan
from chemeleon_amd.finish import finish_atoms
from chemeleon_amd.primitive import RECORD_BYTES, PrimitivePlan, PrimitiveReport
from tests import prim_cases as P
from tests import symmetry_cases as S

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def to_device(nat, types, frac, lat):
    return nat, torch.from_numpy(types).to(DEV), torch.from_numpy(frac).to(DEV), torch.from_numpy(lat).to(DEV)


def device_state(indices):
    return to_device(*P.state(indices))


def run_raw(nat, a, x, lat, bufs=None, cell_rec=None, **n):
    """chm_cell_run + chm_prim_run with every count and pointer overridable -> (rc, bufs): bufs = dict of out
    (uint8 [B*64]), source, new_off, a_p, x_p, lat_p, filled with 0xAB before the run."""
    lib = _lib.load()
    B, N = len(nat), sum(nat)
    st = _lib.stream_handle()
    if cell_rec is None:
        cell_rec = torch.zeros(B * 128, dtype=torch.uint8, device=DEV)
        cells = CellPlan(nat, DEV)  # (kept in a name: the handle must outlive the call)
        rc = lib.chm_cell_run(cells.handle, _lib.ptr(lat), lat.numel(), None, 0, P.SYMPREC, P.ANGLE_TOLERANCE,
                              _lib.ptr(cell_rec), cell_rec.numel(), st)
        assert rc == 0, lib.chm_last_error()
    if bufs is None:
        fill = lambda count, dt: torch.full((count * dt.itemsize,), 0xAB, dtype=torch.uint8, device=DEV).view(dt)  # noqa: E731
        bufs = dict(out=fill(B * RECORD_BYTES, torch.uint8), source=fill(N, torch.int32), new_off=fill(B + 1, torch.int32),
                    a_p=fill(N, torch.int64), x_p=fill(3 * N, torch.float32), lat_p=fill(9 * B, torch.float32))
    plan = n.get("plan") or PrimitivePlan(nat, DEV)
    t = dict(rec=cell_rec, a=a, x=x, lat=lat, **bufs)
    cnt = {k: v.numel() for k, v in t.items()}
    cnt.update({k[2:]: v for k, v in n.items() if k.startswith("n_")})
    t.update({k: None for k in n.get("null", ())})
    t.update(n.get("swap", {}))
    rc = lib.chm_prim_run(
        plan.handle, _lib.ptr(t["rec"], n.get("rec_offset", 0)), cnt["rec"], _lib.ptr(t["a"]), cnt["a"], _lib.ptr(t["x"]),
        cnt["x"], _lib.ptr(t["lat"]), cnt["lat"], n.get("symprec", P.SYMPREC), n.get("angle_tolerance", P.ANGLE_TOLERANCE),
        _lib.ptr(t["out"], n.get("out_offset", 0)), cnt["out"], _lib.ptr(t["source"]), cnt["source"],
        _lib.ptr(t["new_off"]), cnt["new_off"], _lib.ptr(t["a_p"]), cnt["a_p"], _lib.ptr(t["x_p"]), cnt["x_p"],
        _lib.ptr(t["lat_p"]), cnt["lat_p"], st)
    return rc, bufs


def host(bufs, B):
    """The outputs as numpy: records [B,16] int32, source, new_off, a_p [N], x_p [N,3], lat_p [B,3,3]."""
    g = {k: v.cpu().numpy() for k, v in bufs.items()}
    return dict(rec=g["out"].view(np.int32).reshape(B, 16), source=g["source"], new_off=g["new_off"], a_p=g["a_p"],
                x_p=g["x_p"].reshape(-1, 3), lat_p=g["lat_p"].reshape(B, 3, 3))


def per_crystal(h, nat, g):
    """Crystal g's bytes of host(...) output: (record, source rows, lattice, packed types, packed coordinates)."""
    n0 = int(np.sum(nat[:g]))
    lo, hi = int(h["new_off"][g]), int(h["new_off"][g + 1])
    return (h["rec"][g].tobytes(), h["source"][n0:n0 + nat[g]].tobytes(), h["lat_p"][g].tobytes(),
            h["a_p"][lo:hi].tobytes(), h["x_p"][lo:hi].tobytes())


@pytest.fixture(scope="module")
def everything():
    """All cases in one batch, run once: (indices, device state, host outputs)."""
    idx = list(range(len(P.cases())))
    nat, a, x, lat = device_state(idx)
    rc, bufs = run_raw(nat, a, x, lat)
    assert rc == 0, _lib.load().chm_last_error()
    torch.cuda.synchronize()
    return idx, (nat, a, x, lat), host(bufs, len(nat))


def check_against_restatement(h, nat, indices):
    ref = P.reference("float32")
    want_off = np.concatenate([[0], np.cumsum([ref[k]["n_prim"] for k in indices])]).astype(np.int32)
    np.testing.assert_array_equal(h["new_off"], want_off)  # the prefix sums
    n_new = int(want_off[-1])
    assert not h["a_p"][n_new:].any() and not h["x_p"][n_new:].view(np.uint32).any()  # bytes past N' are zero
    for row, k in enumerate(indices):
        want, name = ref[k], P.cases()[k]["name"]
        rec = h["rec"][row]
        got = dict(zip(P.INT_FIELDS, [int(v) for v in rec[:11]]))
        for f in P.INT_FIELDS:
            assert got[f] == int(want[f]), (name, f, got, {q: want[q] for q in P.INT_FIELDS})
        assert rec[11:12].view(np.float32)[0] == np.float32(want["tol"]), name
        assert rec[12] == want["lattice_system"] and not rec[13:].any(), name
        lo, hi = want_off[row], want_off[row + 1]
        same = lambda u, v: np.array_equal(u.view(np.uint32), v.view(np.uint32))  # noqa: E731
        if name == "no_lattice":  # (the NaN of the lattice stays where it was: compare the bits)
            assert np.isnan(h["lat_p"][row]).sum() == 1
        assert same(h["lat_p"][row], want["Lp"]), (name, h["lat_p"][row], want["Lp"])
        assert same(h["x_p"][lo:hi], want["xp"]), (name, h["x_p"][lo:hi], want["xp"])
        np.testing.assert_array_equal(h["a_p"][lo:hi], want["types_p"], err_msg=name)
        n0 = int(np.sum(nat[:row]))
        source = np.full(nat[row], -1, dtype=np.int32)
        source[want["keep"]] = np.arange(len(want["keep"]), dtype=np.int32)
        np.testing.assert_array_equal(h["source"][n0:n0 + nat[row]], source, err_msg=name)


def test_outputs_equal_the_float32_restatement(everything):
    idx, (nat, _, _, _), h = everything
    check_against_restatement(h, nat, idx)
    rep = PrimitiveReport(h["rec"].view(np.uint8), nat)
    by_name = {P.cases()[k]["name"]: row for row, k in enumerate(idx)}
    for name, (n, n_prim, m) in P.EXPECTED.items():  # the textbook table, on the device
        g = by_name[name]
        assert (nat[g], rep.n_prim[g], rep.n_trans[g], rep.flags[g]) == (n, n_prim, m, 0), name
        assert bool(rep.reduced[g]) == (n_prim < n)
    assert rep.halvings[by_name["prim_halving"]] >= 1 and rep.flags[by_name["prim_halving"]] == 0
    assert rep.flags[by_name["thin"]] == P.THIN and rep.flags[by_name["no_lattice"]] == P.NO_LATTICE
    assert not (rep.flags & P.AMBIGUOUS).any()
    assert np.count_nonzero(rep.hnf[by_name["rocksalt8"]]) > 3  # not diagonal


def test_bytes_do_not_depend_on_the_batch(everything):
    idx, (nat, a, x, lat), h = everything
    rc, again = run_raw(nat, a, x, lat)
    assert rc == 0
    h2 = host(again, len(nat))
    for k in h:
        np.testing.assert_array_equal(h2[k].view(np.uint8), h[k].view(np.uint8), err_msg=k)  # a second run
    alone = {}
    for k in idx:  # B = 1: every case alone
        n1, a1, x1, l1 = device_state([k])
        rc, bufs = run_raw(n1, a1, x1, l1)
        assert rc == 0
        h1 = host(bufs, 1)
        check_against_restatement(h1, n1, [k])
        alone[k] = per_crystal(h1, n1, 0)
        assert alone[k] == per_crystal(h, nat, k), P.cases()[k]["name"]
    rng = np.random.default_rng(1)
    for order in (idx[::-1], [int(v) for v in rng.permutation(idx)]):  # the ragged batch in two other orders
        n2, a2, x2, l2 = device_state(order)
        rc, bufs = run_raw(n2, a2, x2, l2)
        assert rc == 0
        ho = host(bufs, len(order))
        check_against_restatement(ho, n2, order)
        for row, k in enumerate(order):
            assert per_crystal(ho, n2, row) == alone[k], P.cases()[k]["name"]


def test_offsets_scan_more_than_one_chunk():
    """k_prim_offsets scans 256 records per round: 600 crystals take three rounds with a carry between them."""
    pool = [P.index_of(n) for n in ("cscl_2x1x1", "one_atom", "rocksalt8", "cscl", "bcc_conventional", "sc_2x2x2", "thin")]
    order = [pool[(k * k + k // 7) % len(pool)] for k in range(600)]
    nat, a, x, lat = device_state(order)
    rc, bufs = run_raw(nat, a, x, lat)
    assert rc == 0
    check_against_restatement(host(bufs, len(order)), nat, order)


def test_run_refuses_bad_arguments():
    lib = _lib.load()
    b = [P.index_of(n) for n in ("cscl_2x1x1", "quartz", "rocksalt8", "thin", "sc_2x2x2")]
    nat, a, x, lat = device_state(b)
    B, N = len(nat), sum(nat)
    plan = PrimitivePlan(nat, DEV)
    rc, good = run_raw(nat, a, x, lat, plan=plan)
    assert rc == 0
    _, bufs = run_raw(nat, a, x, lat, plan=plan)
    torch.cuda.synchronize()
    for v in bufs.values():
        v.view(torch.uint8).fill_(0xAB)
    before = [t.clone() for t in (a, x, lat)]
    pad = torch.zeros(B * 128 + 16, dtype=torch.uint8, device=DEV)
    cases = [({"n_rec": 128 * B - 128}, b"cell records"), ({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"),
             ({"n_lat": 9}, b"lattices"), ({"n_out": 64 * B - 64}, b"out"), ({"n_out": 64 * B + 16}, b"out"),
             ({"n_source": N - 1}, b"source"), ({"n_new_off": B}, b"new_offsets"), ({"n_new_off": B + 2}, b"new_offsets"),
             ({"n_a_p": N + 1}, b"atom_types_out"), ({"n_x_p": 3 * N - 3}, b"frac_out"), ({"n_lat_p": 9 * B + 9}, b"lattices_out"),
             ({"symprec": 0.0}, b"symprec"), ({"symprec": 1.5}, b"symprec"), ({"symprec": float("nan")}, b"symprec"),
             ({"angle_tolerance": -1.0}, b"angle_tolerance"), ({"angle_tolerance": 30.5}, b"angle_tolerance"),
             ({"swap": {"rec": pad}, "rec_offset": 4, "n_rec": 128 * B}, b"16-byte aligned"),
             ({"out_offset": 8}, b"16-byte aligned"),
             ({"swap": {"a_p": a}}, b"atom_types_out must not be"), ({"swap": {"x_p": x}}, b"frac_out must not be"),
             ({"swap": {"lat_p": lat}}, b"lattices_out must not be")]
    cases += [({"null": (k,)}, name) for k, name in (("rec", b"cell records"), ("a", b"atom_types"), ("x", b"frac"),
                                                       ("lat", b"lattices"), ("out", b"out"), ("source", b"source"),
                                                       ("new_off", b"new_offsets"), ("a_p", b"atom_types_out"),
                                                       ("x_p", b"frac_out"), ("lat_p", b"lattices_out"))]
    for kw, name in cases:
        rc, _ = run_raw(nat, a, x, lat, bufs=bufs, plan=plan, **kw)
        assert rc == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    assert lib.chm_prim_run(None, *([None, 0] * 4), 0.1, 10.0, *([None, 0] * 6), None) == -1
    assert b"plan" in lib.chm_last_error()
    torch.cuda.synchronize()
    for v in bufs.values():
        assert bool((v.view(torch.uint8) == 0xAB).all())  # nothing was enqueued, not even the clearing
    for t, was in zip((a, x, lat), before):
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))
    rc, _ = run_raw(nat, a, x, lat, bufs=bufs, plan=plan)
    assert rc == 0, lib.chm_last_error()
    for k in bufs:
        assert torch.equal(bufs[k].view(torch.uint8), good[k].view(torch.uint8)), k
    h = _lib.c_void_p()
    big = (ctypes.c_int32 * 2)(4, 257)
    assert lib.chm_prim_create(big, 2, ctypes.byref(h)) == -3 and b"256" in lib.chm_last_error()  # CHM_E_UNSUPPORTED
    assert lib.chm_prim_create((ctypes.c_int32 * 1)(0), 1, ctypes.byref(h)) == -1


def test_graph_replay_and_eager_are_byte_identical():
    lib = _lib.load()
    b = [P.index_of(n) for n in ("rocksalt8", "one_atom", "cscl_2x3x1", "prim_halving", "no_lattice", "sc_64", "quartz")]
    nat, a, x, lat = device_state(b)
    B = len(nat)
    cells, plan = CellPlan(nat, DEV), PrimitivePlan(nat, DEV)
    rc, eager = run_raw(nat, a, x, lat, plan=plan)
    assert rc == 0
    _, bufs = run_raw(nat, a, x, lat, plan=plan)
    cell_rec = torch.zeros(B * 128, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert lib.chm_cell_run(cells.handle, _lib.ptr(lat), lat.numel(), None, 0, P.SYMPREC, P.ANGLE_TOLERANCE,
                                    _lib.ptr(cell_rec), cell_rec.numel(), _lib.stream_handle()) == 0
            rc, _ = run_raw(nat, a, x, lat, bufs=bufs, cell_rec=cell_rec, plan=plan)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for v in bufs.values():
            v.view(torch.uint8).fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        for k in bufs:
            assert torch.equal(bufs[k].view(torch.uint8), eager[k].view(torch.uint8)), k


def test_python_and_torch_op_return_the_ctypes_bytes(everything):
    from chemeleon_amd import ops as ops_module
    chem = ops_module.load()
    idx, (nat, a, x, lat), h = everything
    before = [t.clone() for t in (a, x, lat)]
    n_new = int(h["new_off"][-1])
    nat_p, a_p, x_p, lat_p, rep = primitive_states(nat, a, x, lat)
    assert nat_p == np.diff(h["new_off"]).tolist() and a_p.shape == (n_new,) and x_p.shape == (n_new, 3)
    np.testing.assert_array_equal(rep.records.view(np.int32), h["rec"])
    np.testing.assert_array_equal(a_p.cpu().numpy(), h["a_p"][:n_new])
    np.testing.assert_array_equal(x_p.cpu().numpy().view(np.uint32), h["x_p"][:n_new].view(np.uint32))
    np.testing.assert_array_equal(lat_p.cpu().numpy().view(np.uint32), h["lat_p"].view(np.uint32))
    assert rep.record(0)["n_prim"] == nat_p[0] and rep.natoms.tolist() == nat
    ta, tx, tl, toff, trec = chem.primitive(a, x, lat, nat, P.SYMPREC, P.ANGLE_TOLERANCE)
    assert trec.shape == (len(nat), 64) and trec.dtype == torch.uint8 and toff.dtype == torch.int32
    assert ta.shape == a.shape and tx.shape == x.shape and tl.shape == lat.shape
    np.testing.assert_array_equal(trec.cpu().numpy().view(np.int32), h["rec"])
    np.testing.assert_array_equal(toff.cpu().numpy(), h["new_off"])
    np.testing.assert_array_equal(ta.cpu().numpy(), h["a_p"])  # (the rows past N' too: zero)
    np.testing.assert_array_equal(tx.cpu().numpy().view(np.uint32), h["x_p"].view(np.uint32))
    np.testing.assert_array_equal(tl.cpu().numpy().view(np.uint32), h["lat_p"].view(np.uint32))
    for t, was in zip((a, x, lat), before):  # the state is never changed in place
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))
    with pytest.raises(RuntimeError, match="shape"):
        chem.primitive(a, x[:-1], lat, nat, 0.1, 10.0)
    with pytest.raises(RuntimeError, match="symprec"):
        chem.primitive(a, x, lat, nat, 2.0, 10.0)
    with pytest.raises(RuntimeError, match="HIP device only"):
        chem.primitive(a.cpu(), x, lat, nat, 0.1, 10.0)
    with pytest.raises(RuntimeError, match="HIP device only"):
        primitive_states(nat, a, x.cpu(), lat)
    with pytest.raises(ValueError, match="chemeleon_amd.Primitive"):
        primitive_states(nat, a, x, lat, Symmetry())
    with pytest.raises(RuntimeError, match="256"):
        primitive_states([257], torch.zeros(257, dtype=torch.int64, device=DEV), torch.zeros(257, 3, device=DEV),
                         torch.eye(3, device=DEV)[None].contiguous())


# --------------------------------------------------------------------------- the caveats, removed
def struct_state(*structs):
    """A device state of (lattice, types, frac) structures."""
    cs = [S._case("s", s) for s in structs]
    return to_device([len(c["types"]) for c in cs], np.concatenate([c["types"] for c in cs]),
                     np.concatenate([c["frac"] for c in cs]), np.stack([c["lattice"] for c in cs]))


def test_symmetry_of_a_supercell_is_that_of_its_primitive_cell():
    state = device_state([P.index_of("cscl_2x1x1")])
    as_given = symmetry_states(*state)
    assert as_given.system[0] == "tetragonal" and as_given.n_trans[0] == 2  # as today
    nat_p, a_p, x_p, lat_p, rep = primitive_states(*state)
    assert nat_p == [2] and rep.reduced[0] and rep.n_trans[0] == 2
    prim = symmetry_states(nat_p, a_p, x_p, lat_p)
    assert prim.system[0] == "cubic" and prim.n_trans[0] == 1 and prim.n_pg[0] == 48


def test_match_and_grouping_merge_a_supercell_with_its_primitive_cell():
    base = S._base_structures()
    L2, t2, f2 = base["rocksalt_primitive"]
    ref = Reference([2], t2, f2.astype(np.float32), L2.astype(np.float32)[None])
    conventional = struct_state(base["rocksalt8"])
    before = match_states(*conventional, Match(ref))
    assert not before.matched[0] and before.flags[0] == match_module.SIZE
    nat_p, a_p, x_p, lat_p, _ = primitive_states(*conventional)
    after = match_states(nat_p, a_p, x_p, lat_p, Match(ref))
    assert nat_p == [2] and after.matched[0] and after.flags[0] == 0 and after.rms[0] < 1e-4
    for order in (("rocksalt_primitive", "rocksalt8"), ("rocksalt8", "rocksalt_primitive")):
        nat, a, x, lat = struct_state(*[base[n] for n in order])
        assert match_group_states(nat, a, x, lat).n_groups == 2  # as today: unequal atom counts never merge
        atoms, reports = finish_atoms(nat, a, x, lat, primitive=Primitive(), dedup=MatchDedup())
        assert reports["dedup"].n_groups == 1 and reports["dedup"].group.tolist() == [0, 0]
        assert reports["primitive"].n_prim.tolist() == [2, 2]
        assert reports["primitive"].reduced.tolist() == [n == "rocksalt8" for n in order]
        assert len(atoms) == 1 and len(atoms[0]) == 2 and sorted(atoms[0].numbers.tolist()) == [11, 17]
        info = atoms[0].info["primitive"]
        assert info["index"] == 0 and info["n_prim"] == 2 and info["reduced"] == (order[0] == "rocksalt8")
        assert abs(abs(np.linalg.det(np.asarray(atoms[0].cell, dtype=np.float64))) - 5.6 ** 3 / 4) < 1e-3


def test_without_the_keyword_nothing_of_it_runs():
    from chemeleon_amd import primitive as primitive_module
    from chemeleon_amd.screening import selected_atoms
    base = S._base_structures()
    nat, a, x, lat = struct_state(base["rocksalt_primitive"], base["rocksalt8"], base["cscl_2x1x1"])
    plans = len(primitive_module._plans)
    atoms, reports = finish_atoms(nat, a, x, lat, symmetry=Symmetry(), dedup=MatchDedup())
    assert set(reports) == {"symmetry", "dedup"} and len(primitive_module._plans) == plans
    assert [len(at) for at in atoms] == [2, 8, 4] and reports["dedup"].n_groups == 3
    assert reports["symmetry"].system.tolist() == ["cubic", "cubic", "tetragonal"]
    for at, other in zip(atoms, selected_atoms(nat, a, x, lat, [0, 1, 2])):  # the structures of the state as it is
        assert "primitive" not in at.info
        np.testing.assert_array_equal(np.asarray(at.numbers), np.asarray(other.numbers))
        np.testing.assert_array_equal(at.get_scaled_positions(), other.get_scaled_positions())
        np.testing.assert_array_equal(np.asarray(at.cell), np.asarray(other.cell))
    with_it, reports = finish_atoms(nat, a, x, lat, symmetry=Symmetry(), primitive=Primitive())
    assert list(reports) == ["primitive", "symmetry"] and [len(at) for at in with_it] == [2, 2, 2]
    assert reports["symmetry"].system.tolist() == ["cubic"] * 3 and reports["symmetry"].n_trans.tolist() == [1] * 3


def test_sample_refuses_up_front():
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    cfg = default_config()
    cfg["timesteps"] = 100
    m = Chemeleon(cfg)  # (never moved to the device: every refusal comes before anything is sampled)
    with pytest.raises(ValueError, match="chemeleon_amd.Primitive"):
        m.sample(None, 6, 2, primitive="yes")
    with pytest.raises(ValueError, match="finished structures"):
        m.sample(None, 6, 2, stream=True, primitive=Primitive())
    with pytest.raises(ValueError, match="finished structures"):
        m.sample(None, 6, 2, return_trajectory=True, primitive=Primitive())
    with pytest.raises(ValueError, match="at most 256 atoms"):
        m.sample(None, 257, 1, primitive=Primitive())
    assert m.last_primitive is None
