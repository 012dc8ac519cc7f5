"""Crystal system with the atoms on the device (chemeleon_amd.symmetry, csrc/symm.hip) against the numpy
restatements of tests/symmetry_cases.py: the records (every integer field and tol, bit for bit) against the
float32 restatement, alone, in batches and run twice; the operations output checked in float64; the argument
checks; stream capture; the Python and torch-op layers; and sample(symmetry=...) with the other legs.

The cases keep a margin of symmetry_cases.MARGIN between every distance test and its tolerance in float64
(tests/test_symmetry_cases.py), so the float32 arithmetic decides nothing differently from the definition."""

import numpy as np
import pytest
import torch

from chemeleon_amd import Cell, Dedup, Screen, Symmetry, _lib, cell_states, dedup_states, screen_states, symmetry_states
from chemeleon_amd.cell import SYSTEMS as CELL_SYSTEMS
from chemeleon_amd.cell import CellPlan
from chemeleon_amd.config import default_config
from chemeleon_amd.symmetry import (CRYSTAL_SYSTEMS, MAX_OPS, RECORD_BYTES, SymmetryPlan, SymmetryReport,
                                    candidate_matrix)
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from tests import symmetry_cases as S

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def device_state(indices):
    nat, types, frac, lat = S.state(indices)
    return nat, torch.from_numpy(types).to(DEV), torch.from_numpy(frac).to(DEV), torch.from_numpy(lat).to(DEV)


def run_raw(nat, a, x, lat, require=None, ops=False, out=None, ops_out=None, cell_rec=None, **n):
    """chm_cell_run + chm_symm_run with every count and pointer overridable -> (rc, out, ops)."""
    lib = _lib.load()
    B = len(nat)
    st = _lib.stream_handle()
    if cell_rec is None:
        cell_rec = torch.zeros(B * 128, dtype=torch.uint8, device=DEV)
        cells = CellPlan(nat, DEV)  # (kept in a name: the handle must outlive the call)
        rc = lib.chm_cell_run(cells.handle, _lib.ptr(lat), lat.numel(), None, 0, S.SYMPREC,
                              S.ANGLE_TOLERANCE, _lib.ptr(cell_rec), cell_rec.numel(), st)
        assert rc == 0, lib.chm_last_error()
    if out is None:
        out = torch.full((B * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    if ops and ops_out is None:
        ops_out = torch.full((B * MAX_OPS * 16,), 0xAB, dtype=torch.uint8, device=DEV)
    plan = n.get("plan") or SymmetryPlan(nat, DEV)
    ptrs = dict(rec=cell_rec, a=a, x=x, lat=lat, out=out)
    ptrs.update({k: None for k in n.get("null", ())})
    rc = lib.chm_symm_run(
        plan.handle, _lib.ptr(ptrs["rec"]), n.get("n_rec", cell_rec.numel()), _lib.ptr(ptrs["a"]),
        n.get("n_a", a.numel()), _lib.ptr(ptrs["x"]), n.get("n_x", x.numel()), _lib.ptr(ptrs["lat"]),
        n.get("n_l", lat.numel()), _lib.ptr(require), n.get("n_r", 0 if require is None else require.numel()),
        n.get("symprec", S.SYMPREC), n.get("angle_tolerance", S.ANGLE_TOLERANCE), _lib.ptr(ptrs["out"]),
        n.get("n_o", out.numel()), _lib.ptr(ops_out), n.get("n_ops", 0 if ops_out is None else ops_out.numel()), st)
    return rc, out, ops_out


@pytest.fixture(scope="module")
def everything():
    """All cases in one batch: (indices, device state, records [B,64], operation slots [B,48,16]), run once."""
    idx = list(range(len(S.cases())))
    nat, a, x, lat = device_state(idx)
    rc, out, ops = run_raw(nat, a, x, lat, ops=True)
    assert rc == 0, _lib.load().chm_last_error()
    return idx, (nat, a, x, lat), out.cpu().numpy().reshape(-1, RECORD_BYTES), ops.cpu().numpy().reshape(-1, MAX_OPS, 16)


def check_records(records, indices, require=-1):
    ref = S.reference("float32", require)
    rep = SymmetryReport(records)
    ints = records.view(np.int32)
    for row, k in enumerate(indices):
        want, name = ref[k], S.cases()[k]["name"]
        got = dict(zip(S.INT_FIELDS, [int(v) for v in ints[row, :14]]))
        # the record's order: system, n_sym, n_trans, n_pg, n_proper, n2, n3, n4, n6, inversion, halvings, flags,
        # n_pivot, lattice_system
        for f in S.INT_FIELDS:
            assert got[f] == int(want[f]), (name, f, got, {q: want[q] for q in S.INT_FIELDS})
        assert records.view(np.float32)[row, 14] == np.float32(want["tol"]), name
        assert ints[row, 15] == 0, name
        assert rep.code[row] == want["system"]


def test_records_equal_the_float32_restatement(everything):
    idx, _, records, _ = everything
    check_records(records, idx)
    rep = SymmetryReport(records)
    by_name = {S.cases()[k]["name"]: row for row, k in enumerate(idx)}
    for name, (system, n_pg, inv, n_trans) in S.EXPECTED.items():  # the textbook table, on the device
        g = by_name[name]
        assert (rep.system[g], rep.n_pg[g], int(rep.inversion[g]), rep.n_trans[g]) == (system, n_pg, inv, n_trans), name
    assert rep.lattice_system[by_name["quartz"]] == "hexagonal" and rep.system[by_name["quartz"]] == "trigonal"
    assert rep.halvings[by_name["one_halving"]] >= 1
    assert rep.flags[by_name["thin"]] == S.THIN and rep.flags[by_name["no_lattice"]] == S.NO_LATTICE


def test_bytes_do_not_depend_on_the_batch(everything):
    idx, (nat, a, x, lat), records, _ = everything
    rc, again, _ = run_raw(nat, a, x, lat)
    assert rc == 0
    np.testing.assert_array_equal(again.cpu().numpy().reshape(-1, RECORD_BYTES), records)  # a second run
    b65 = S.batch(65)
    rc, out, _ = run_raw(*device_state(b65))
    assert rc == 0
    got65 = out.cpu().numpy().reshape(65, RECORD_BYTES)
    check_records(got65, b65)
    np.testing.assert_array_equal(got65, records[b65])
    for k in idx:  # B = 1: every case alone
        rc, out, _ = run_raw(*device_state([k]))
        assert rc == 0
        np.testing.assert_array_equal(out.cpu().numpy(), records[k], err_msg=S.cases()[k]["name"])


def test_operations_map_the_structure_onto_itself(everything):
    idx, _, records, slots = everything
    ref = S.reference("float32")
    rep = SymmetryReport(records, slots)
    for row, k in enumerate(idx):
        want, c = ref[k], S.cases()[k]
        index = slots[row].view(np.int32)[:, 0]
        used = int((index >= 0).sum())
        assert used == rep.n_pg[row], c["name"]
        assert np.all(index[:used] >= 0) and np.all(np.diff(index[:used]) > 0)  # packed, ascending
        assert np.all(slots[row, used:].view(np.int32)[:, 0] == -1) and not slots[row, used:, 4:].any()
        if not used:
            continue
        ids, Ws, ts = rep.operations[row]
        assert [o[0] for o in want["ops"]] == ids.tolist(), c["name"]
        np.testing.assert_array_equal(np.stack([o[1] for o in want["ops"]]).view(np.uint32), ts.view(np.uint32))
        assert set(ids.tolist()) <= set(want["W_index"].tolist())  # each W is an accepted lattice operation
        x, L = want["xr"].astype(np.float64), want["Lr"].astype(np.float64)
        same = c["types"][:, None] == c["types"][None, :]
        for W, t in zip(Ws, ts):
            assert np.array_equal(W, candidate_matrix(S.candidate_index(W)))
            d = (x @ W.astype(np.float64) + t.astype(np.float64))[:, None, :] - x[None, :, :]
            d -= np.rint(d)
            dist = np.where(same, np.linalg.norm(d @ L, axis=-1), np.inf).min(axis=1)
            assert dist.max() <= float(rep.tol[row]) * (1 + S.MARGIN), (c["name"], dist.max())


def test_require_one_name_and_per_crystal(everything):
    idx, (nat, a, x, lat), records, _ = everything
    free = SymmetryReport(records)
    rq = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    rc, out, _ = run_raw(nat, a, x, lat, require=rq)
    assert rc == 0
    got = out.cpu().numpy().reshape(-1, RECORD_BYTES)
    check_records(got, idx, require=6)
    assert np.array_equal(SymmetryReport(got).mismatch, free.code != 6)
    names = [CRYSTAL_SYSTEMS[(k + (k % 3 == 0)) % 7] if free.code[k] < 0 else
             CRYSTAL_SYSTEMS[(free.code[k] + (k % 3 == 0)) % 7] for k in range(len(idx))]
    rep = symmetry_states(nat, a, x, lat, Symmetry(require=names))
    assert np.array_equal(rep.mismatch, np.array([CRYSTAL_SYSTEMS.index(n) for n in names]) != free.code)
    assert np.array_equal(rep.records[:, :44], records[:, :44]) and np.array_equal(rep.records[:, 48:], records[:, 48:])
    assert 0 < rep.mismatch.sum() < len(idx) and not rep.valid[rep.mismatch].any()


def test_run_refuses_bad_arguments():
    lib = _lib.load()
    b = S.batch(5)
    nat, a, x, lat = device_state(b)
    B, N = len(nat), sum(nat)
    plan = SymmetryPlan(nat, DEV)
    rc, good, good_ops = run_raw(nat, a, x, lat, ops=True, plan=plan)
    assert rc == 0
    out = torch.full((B * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    ops = torch.full((B * MAX_OPS * 16,), 0xAB, dtype=torch.uint8, device=DEV)
    rq = torch.zeros(B, dtype=torch.int32, device=DEV)
    before = [t.clone() for t in (a, x, lat)]
    for kw, name in [({"n_rec": 128 * B - 128}, b"cell records"), ({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"),
                     ({"n_l": 9}, b"lattices"), ({"n_r": B - 1}, b"require"), ({"n_r": 0}, b"require"),
                     ({"n_o": 64 * B - 64}, b"out"), ({"n_o": 64 * B + 16}, b"out"), ({"n_ops": 768 * B - 16}, b"ops"),
                     ({"n_ops": 0}, b"ops"), ({"symprec": 0.0}, b"symprec"), ({"symprec": 1.5}, b"symprec"),
                     ({"symprec": float("nan")}, b"symprec"), ({"angle_tolerance": -1.0}, b"angle_tolerance"),
                     ({"angle_tolerance": 30.5}, b"angle_tolerance"), ({"null": ("rec",)}, b"cell records"),
                     ({"null": ("a",)}, b"atom_types"), ({"null": ("x",)}, b"frac"), ({"null": ("lat",)}, b"lattices"),
                     ({"null": ("out",)}, b"out")]:
        rc, _, _ = run_raw(nat, a, x, lat, require=rq, out=out, ops_out=ops, plan=plan, **kw)
        assert rc == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    rc, _, _ = run_raw(nat, a, x, lat, out=out, plan=plan, n_r=1)
    assert rc == -1 and b"require" in lib.chm_last_error()
    rc, _, _ = run_raw(nat, a, x, lat, out=out, plan=plan, n_ops=768 * B)
    assert rc == -1 and b"ops" in lib.chm_last_error()
    assert lib.chm_symm_run(None, *([None, 0] * 5), 0.1, 10.0, None, 0, None, 0, None) == -1
    assert b"plan" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((ops == 0xAB).all())  # nothing was enqueued
    for t, was in zip((a, x, lat), before):
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))
    rc, out, ops = run_raw(nat, a, x, lat, out=out, ops_out=ops, plan=plan)
    assert rc == 0, lib.chm_last_error()
    assert torch.equal(out, good) and torch.equal(ops, good_ops)
    h = _lib.c_void_p()
    import ctypes
    big = (ctypes.c_int32 * 2)(4, 257)
    assert lib.chm_symm_create(big, 2, ctypes.byref(h)) == -3 and b"256" in lib.chm_last_error()  # CHM_E_UNSUPPORTED


def test_graph_replay_and_eager_are_byte_identical():
    lib = _lib.load()
    b = S.batch(9)
    nat, a, x, lat = device_state(b)
    B = len(nat)
    cells, plan = CellPlan(nat, DEV), SymmetryPlan(nat, DEV)
    rc, eager, eager_ops = run_raw(nat, a, x, lat, ops=True, plan=plan)
    assert rc == 0
    cell_rec = torch.zeros(B * 128, dtype=torch.uint8, device=DEV)
    out, ops = torch.zeros_like(eager), torch.zeros_like(eager_ops)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert lib.chm_cell_run(cells.handle, _lib.ptr(lat), lat.numel(), None, 0, S.SYMPREC, S.ANGLE_TOLERANCE,
                                    _lib.ptr(cell_rec), cell_rec.numel(), _lib.stream_handle()) == 0
            rc, _, _ = run_raw(nat, a, x, lat, out=out, ops_out=ops, cell_rec=cell_rec, plan=plan)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(0x5C)
        ops.fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(ops, eager_ops)


def test_python_and_torch_op_return_the_ctypes_bytes(everything):
    from chemeleon_amd import ops as ops_module
    chem = ops_module.load()
    idx, (nat, a, x, lat), records, slots = everything
    rep = symmetry_states(nat, a, x, lat, operations=True)
    np.testing.assert_array_equal(rep.records, records)
    np.testing.assert_array_equal(rep.operation_slots, slots)
    assert symmetry_states(nat, a, x, lat).operations is None
    rec, ops = chem.symmetry(a, x, lat, nat, None, S.SYMPREC, S.ANGLE_TOLERANCE, True)
    assert rec.shape == (len(nat), 64) and rec.dtype == torch.uint8 and ops.shape == (len(nat), 48, 16)
    np.testing.assert_array_equal(rec.cpu().numpy(), records)
    np.testing.assert_array_equal(ops.cpu().numpy(), slots)
    rq = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    rec, ops = chem.symmetry(a, x, lat, nat, rq, S.SYMPREC, S.ANGLE_TOLERANCE, False)
    assert ops.shape == (0, 48, 16)
    assert np.array_equal(SymmetryReport(rec.cpu().numpy()).mismatch, SymmetryReport(records).code != 6)
    with pytest.raises(RuntimeError, match="shape"):
        chem.symmetry(a, x[:-1], lat, nat, None, 0.1, 10.0, False)
    with pytest.raises(RuntimeError, match="symprec"):
        chem.symmetry(a, x, lat, nat, None, 2.0, 10.0, False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        chem.symmetry(a.cpu(), x, lat, nat, None, 0.1, 10.0, False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        symmetry_states(nat, a, x.cpu(), lat)


# --------------------------------------------------------------------------- Chemeleon.sample(symmetry=...)
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
    """(kw, natoms, a, x, lat, every structure): the final state of the 4 x 6 run, computed once."""
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


def test_sample_returns_only_the_required_system(model100, final):
    kw, natoms, a, x, lat, every = final
    free = symmetry_states(natoms, a, x, lat)
    atoms = model100.sample(None, 6, 4, symmetry=Symmetry(), **kw)
    np.testing.assert_array_equal(model100.last_symmetry.records, free.records)  # the whole batch
    assert [at.info["symmetry"]["index"] for at in atoms] == [0, 1, 2, 3]
    absent = next(s for s in CRYSTAL_SYSTEMS if s not in set(free.system.tolist()))
    for name in sorted(set(free.system.tolist()) - {""}) + [absent]:
        atoms = model100.sample(None, 6, 4, symmetry=Symmetry(require=name), **kw)
        keep = np.flatnonzero(free.system == name).tolist()
        assert [at.info["symmetry"]["index"] for at in atoms] == keep, name
        assert len(model100.last_symmetry) == 4
        assert np.array_equal(model100.last_symmetry.mismatch, free.system != name)
        for at, g in zip(atoms, keep):
            same_structure(at, every[g])
            assert at.info["symmetry"]["system"] == name and at.info["symmetry"]["valid"]
    # one name per crystal: every crystal's own system, but a wrong one at index 1, whatever was sampled
    names = [str(s) or "cubic" for s in free.system]
    names[1] = next(n for n in CRYSTAL_SYSTEMS if n != free.system[1])
    atoms = model100.sample(None, 6, 4, symmetry=Symmetry(require=names), **kw)
    keep = [g for g in range(4) if g != 1 and free.system[g]]
    assert [at.info["symmetry"]["index"] for at in atoms] == keep
    assert np.array_equal(model100.last_symmetry.mismatch, np.array(names) != free.system)
    assert model100.last_symmetry.mismatch[1] and np.array_equal(model100.last_symmetry.code, free.code)
    for at, g in zip(atoms, keep):
        same_structure(at, every[g])
        assert at.info["symmetry"]["system"] == names[g] and not at.info["symmetry"]["failed"]
    with pytest.raises(ValueError, match="lists 3 crystal systems"):
        model100.sample(None, 6, 4, symmetry=Symmetry(require=names[:3]), **kw)
    with pytest.raises(ValueError, match="at most 256 atoms"):  # refused before anything is sampled
        model100.sample(None, 257, 1, symmetry=Symmetry(), **kw)


def test_without_the_keyword_nothing_changes(model100, final):
    from chemeleon_amd import symmetry as symmetry_module
    kw, natoms, a, x, lat, every = final
    plans = len(symmetry_module._plans)
    model100.last_symmetry = None
    atoms = model100.sample(None, 6, 4, **kw)
    assert model100.last_symmetry is None and len(symmetry_module._plans) == plans
    assert len(atoms) == 4
    for at, other in zip(atoms, every):
        same_structure(at, other)  # (bit for bit the state of sample_states on the same seed)
        assert "symmetry" not in (getattr(at, "info", None) or {})
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, stream=True, symmetry=Symmetry())
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, return_trajectory=True, symmetry=Symmetry())
    with pytest.raises(ValueError, match="chemeleon_amd.Symmetry"):
        model100.sample(None, 6, 2, symmetry="cubic")


def test_sample_runs_screen_cell_symmetry_then_dedup(model100, final):
    kw, natoms, a, x, lat, every = final
    free = screen_states(natoms, a, x, lat, Screen(max_length=1e6, min_distance=1e-6))
    d = float(np.sort(free.dmin)[1])  # the closest-packed sample fails the screen
    screen = Screen(max_length=1e6, min_distance=d)
    screened = screen_states(natoms, a, x, lat, screen)
    cells, syms = cell_states(natoms, a, x, lat), symmetry_states(natoms, a, x, lat)
    # each leg gets one crystal of its own to exclude, whatever was sampled: the screen crystal s (above); the cell
    # and the symmetry a list with every crystal's own system but a wrong one at c and at w; crystal r passes all
    s_ = int(np.flatnonzero(~screened.valid)[0])
    good = [g for g in range(4) if g != s_ and cells.system[g] and syms.system[g]]
    assert (~screened.valid).sum() == 1 and len(good) >= 2
    r, w = good[0], good[-1]
    c = next(g for g in range(4) if g not in (s_, r, w))
    lattice_names = [str(v) or "cubic" for v in cells.system]
    lattice_names[c] = next(n for n in CELL_SYSTEMS if n != cells.system[c])
    names = [str(v) or "cubic" for v in syms.system]
    names[w] = next(n for n in CRYSTAL_SYSTEMS if n != syms.system[w])
    atoms = model100.sample(None, 6, 4, screen=screen, cell=Cell(require=lattice_names), symmetry=Symmetry(require=names),
                            dedup=Dedup(), **kw)
    srep, crep, yrep, drep = model100.last_screen, model100.last_cell, model100.last_symmetry, model100.last_dedup
    off_lattice, missed = np.array(lattice_names) != cells.system, np.array(names) != syms.system
    failed = ~srep.valid | off_lattice | missed
    assert np.array_equal(srep.valid, screened.valid)
    assert np.array_equal(crep.mismatch, off_lattice) and crep.mismatch[c] and not crep.mismatch[[r, w]].any()
    assert np.array_equal(yrep.mismatch, missed) and yrep.mismatch[w] and not yrep.mismatch[r]
    assert np.array_equal(yrep.code, syms.code)  # the symmetry leg saw the whole batch, the other legs' failures too
    want = dedup_states(natoms, a, x, lat, Dedup(), failed)
    np.testing.assert_array_equal(drep.group, want.group)
    assert np.all(drep.group[[s_, c, w]] == -1) and drep.group[r] >= 0  # the failures of all three take no part
    keep = np.flatnonzero(want.representative).tolist()
    assert keep == [r]
    assert [at.info["dedup"]["index"] for at in atoms] == keep
    for at, g in zip(atoms, keep):
        same_structure(at, every[g])
        assert at.info["screen"]["valid"] and at.info["cell"]["system"] == lattice_names[g]
        assert at.info["symmetry"]["system"] == names[g] and at.info["symmetry"]["index"] == g
