"""Lattice system and reduced cell on the device (csrc/cell.hip, chm_cell_*, chemeleon_amd.cell) against the
float64 restatement of tests/cell_cases.py: the records of batches of 1, 3 and 65 crystals, the reduced cells and
coordinates of reduce_states, determinism and graph capture, the argument checks, the torch op, and
Chemeleon.sample(cell=...).

Exact: code, n_ops, (n2, n3, n4, n6), halvings, the reduction's passes and T, and every flag (the
margin condition of tests/test_cell_cases.py keeps every candidate 1e-3 of the tolerance away from a decision,
hundreds of times the float32 error of a length or an angle of these cells). Gates, as in tests/test_gpu_screen.py:
a + b + c within 16 * 2^-24 * (a + b + c), the volume within 16 * 2^-24 * a * b * c, angles within 1e-3 degrees
on the cases marked tie-free (elsewhere equivalent reduced cells differ in their angles by a symmetry).

reduce_states: with x' and Lr from the device, f = (x' Lr - x L) Lr^-1 in float64 must be integers within
8 * 2^-24 = 4.8e-7 (fractional units): x' is a float64 value rounded once to float32 in [0, 1) (at most 2^-25),
and each entry of Lr is T L rounded once (2^-25 relative), which moves x' Lr Lr_exact^-1 by at most
2^-25 * sum_k |Lr_k| |Lr^-1|, under 9 * 2^-25 for a reduced cell (angles between 60 and 120 degrees)."""

import numpy as np
import pytest
import torch

from chemeleon_amd import Cell, Dedup, Screen, _lib, cell_states, dedup_states, reduce_states, screen_states
from chemeleon_amd.cell import RECORD_BYTES, CellPlan, CellReport
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from tests import cell_cases as C

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
DECIDED = C.DEGENERATE | C.NONFINITE | C.AMBIGUOUS | C.MISMATCH | C.NOT_REDUCED
FRAC_BOUND = 8 * 2.0 ** -24


def lattices_of(idx):
    return torch.from_numpy(np.stack([C.cases()[k]["lattice"] for k in idx])).to(DEV)


@pytest.fixture(scope="module")
def batch65():
    idx = C.batch(65)
    lat = lattices_of(idx)
    x = torch.from_numpy(np.random.default_rng(5).random((65, 3), dtype=np.float32)).to(DEV)
    return idx, x, lat


@pytest.fixture(scope="module")
def plan65():
    return CellPlan([1] * 65, DEV)


def run_raw(plan, lat, require=None, out=None, **n):
    """chm_cell_run with every count overridable -> (rc, out)."""
    B = len(plan.natoms)
    if out is None:
        out = torch.zeros(B * RECORD_BYTES, dtype=torch.uint8, device=DEV)
    rc = _lib.load().chm_cell_run(
        plan.handle, _lib.ptr(lat), n.get("n_l", lat.numel()), _lib.ptr(require),
        n.get("n_r", 0 if require is None else require.numel()), n.get("symprec", C.SYMPREC),
        n.get("angle_tolerance", C.ANGLE_TOLERANCE), _lib.ptr(out), n.get("n_o", out.numel()), _lib.stream_handle())
    return rc, out


def apply_raw(plan, rec, x, lat, x_out, lat_out, **n):
    return _lib.load().chm_cell_apply(
        plan.handle, _lib.ptr(rec), n.get("n_rec", rec.numel()), _lib.ptr(x), n.get("n_x", x.numel()), _lib.ptr(lat),
        n.get("n_l", lat.numel()), _lib.ptr(x_out), n.get("n_xo", x_out.numel()), _lib.ptr(lat_out),
        n.get("n_lo", lat_out.numel()), _lib.stream_handle())


def check_records(rep, idx, latr, require=-1):
    """`latr`: the reduced lattices [B,3,3] (numpy) that reduce_states returned for the same batch."""
    cs, ref = C.cases(), C.reference(require)
    assert len(rep) == len(idx) == len(latr)
    for g, k in enumerate(idx):
        c, r = cs[k], ref[k]
        name = c["name"]
        got = (int(rep.code[g]), int(rep.n_ops[g]), tuple(int(v) for v in rep.orders[g]), int(rep.halvings[g]),
               int(rep.flags[g]) & DECIDED)
        want = (r["code"], r["counts"][0], tuple(r["counts"][1:]), r["halvings"], r["flags"] & DECIDED)
        print(f"{name}: {got} ref {want} passes {rep.passes[g]} ref {r['passes']}")
        assert got == want, name
        # the reduction is the same float64 expression in both, so its passes and T are equal as well
        assert int(rep.passes[g]) == r["passes"], name
        T = rep.transform[g].astype(np.int64)
        assert np.array_equal(T, r["transform"]), name
        assert round(float(np.linalg.det(T.astype(np.float64)))) == 1, name
        L = c["lattice"].astype(np.float64)
        if r["flags"] & C.NONFINITE:
            # the input cell as in k_screen: the rows without the NaN keep their lengths, and the lattice is copied
            assert np.array_equal(T, np.eye(3, dtype=np.int64)), name
            with np.errstate(invalid="ignore"):
                ln = np.sqrt((L * L).sum(1))
            assert np.isnan(ln).any() and np.isfinite(ln).any(), name
            np.testing.assert_allclose(rep.lengths[g], ln, rtol=0, atol=16 * 2.0 ** -24 * float(np.nansum(ln)),
                                       equal_nan=True, err_msg=name)
            assert np.array_equal(latr[g].view(np.uint32), c["lattice"].view(np.uint32)), name
            continue
        # T L equals the returned lattice to float32 rounding (half an ulp of the entry, and the cancellation of a
        # sheared cell's large entries in float64: 2^-52 of the largest product)
        TL = T.astype(np.float64) @ L
        slack = 2.0 ** -24 * np.abs(TL) + 2.0 ** -50 * float(np.abs(T).max()) * float(np.abs(L).max())
        assert np.all(np.abs(TL - latr[g].astype(np.float64)) <= slack), name
        ln = r["lengths"]
        gate = 16 * 2.0 ** -24 * float(ln.sum())
        print(f"   a+b+c {abs(float(rep.lengths[g].astype(np.float64).sum()) - ln.sum()) / gate:.3f} gate, volume "
              f"{abs(float(rep.volume[g]) - r['volume']) / (16 * 2.0 ** -24 * float(np.prod(ln))):.3f} gate, angles "
              f"{np.abs(rep.angles[g] - r['angles']).max():.2e} deg")
        assert abs(float(rep.lengths[g].astype(np.float64).sum()) - float(ln.sum())) <= gate, name
        assert abs(float(rep.volume[g]) - r["volume"]) <= 16 * 2.0 ** -24 * float(np.prod(ln)), name
        if r["flags"] & C.DEGENERATE:
            assert np.array_equal(T, np.eye(3, dtype=np.int64)), name
            np.testing.assert_allclose(rep.lengths[g], ln, rtol=0, atol=gate, err_msg=name)
            continue
        if r["flags"] & C.NOT_REDUCED:
            continue
        a, b, c3 = (float(v) for v in rep.lengths[g])
        assert a <= b * (1 + 1e-5) and b <= c3 * (1 + 1e-5), name
        if c["tie_free"]:
            np.testing.assert_allclose(rep.lengths[g], ln, rtol=0, atol=gate, err_msg=name)
            np.testing.assert_allclose(rep.angles[g], r["angles"], rtol=0, atol=1e-3, err_msg=name)


@pytest.mark.parametrize("B", [1, 3, 65])
def test_records_match_float64(B):
    idx = C.batch(B)
    lat = lattices_of(idx)
    x = torch.zeros(B, 3, device=DEV)
    _, latr, rep = reduce_states([1] * B, None, x, lat)
    np.testing.assert_array_equal(rep.records, cell_states([1] * B, None, x, lat).records)
    check_records(rep, idx, latr.cpu().numpy())


def test_required_systems_set_the_mismatch_bit(batch65):
    idx, x, lat = batch65
    _, latr, rep = reduce_states([1] * 65, None, x, lat, Cell(require="cubic"))
    check_records(rep, idx, latr.cpu().numpy(), require=6)
    assert 0 < rep.mismatch.sum() < 65 and np.array_equal(rep.mismatch, rep.code != 6)
    # one name per crystal: every crystal's own system, except the flagged ones, which have none and never match
    names = [C.SYSTEMS[max(C.cases()[k]["system"], 0)] for k in idx]
    per = cell_states([1] * 65, None, x, lat, Cell(require=names))
    assert np.array_equal(per.mismatch, np.array([C.cases()[k]["system"] < 0 for k in idx]))
    assert np.array_equal(per.valid, ~per.mismatch)


def test_cubic_accepts_48_and_triclinic_2(batch65):
    """The exactly cubic cell accepts 48 candidates and a generic triclinic cell 2, no more. 19 683 = 76 * 256 + 227,
    so the last pass has idle lanes; this does not guard them by itself: the indices 19 683 .. 19 711 decode (mod 3^9)
    to matrices with two equal rows, whose determinant is 0, so they would be rejected even if they were walked.
    What it pins is that nothing beyond the holohedry is counted at either end of the table."""
    idx, x, lat = batch65
    rep = cell_states([1] * 65, None, x, lat)
    by_name = {C.cases()[k]["name"]: g for g, k in enumerate(idx)}
    assert rep.n_ops[by_name["cubic"]] == 48 and rep.n_ops[by_name["triclinic"]] == 2
    assert rep.system[by_name["cubic"]] == "cubic" and rep.system[by_name["triclinic"]] == "triclinic"


@pytest.mark.parametrize("natoms", [[1], [5, 64, 65], [257]])
def test_reduce_states(natoms):
    rng = np.random.default_rng(sum(natoms))
    moved = [k for k, c in enumerate(C.cases()) if c["name"].endswith(("_u0", "_u1", "_u2"))]
    idx = [moved[int(v)] for v in rng.choice(len(moved), size=len(natoms), replace=False)]
    lat = lattices_of(idx)
    N = sum(natoms)
    x = torch.from_numpy(rng.random((N, 3), dtype=np.float32)).to(DEV)
    a = torch.full((N,), 22, dtype=torch.long, device=DEV)
    x0, lat0 = x.clone(), lat.clone()
    xr, latr, rep = reduce_states(natoms, a, x, lat)
    assert xr.is_cuda and latr.is_cuda and xr.shape == x.shape and latr.shape == lat.shape
    assert xr.data_ptr() != x.data_ptr() and latr.data_ptr() != lat.data_ptr()
    assert torch.equal(x, x0) and torch.equal(lat, lat0)  # the inputs are unchanged
    np.testing.assert_array_equal(rep.records, cell_states(natoms, a, x, lat).records)
    xr, latr = xr.cpu().numpy(), latr.cpu().numpy()
    assert np.all(xr >= 0) and np.all(xr < 1)
    offs = np.concatenate([[0], np.cumsum(natoms)])
    worst = 0.0
    for g, k in enumerate(idx):
        L = C.cases()[k]["lattice"].astype(np.float64)
        T = rep.transform[g].astype(np.float64)
        assert round(float(np.linalg.det(T))) == 1 and np.abs(T).max() > 1  # (these cells do need reducing)
        Lr = latr[g].astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(Lr, axis=1), rep.lengths[g], rtol=0,
                                   atol=16 * 2.0 ** -24 * float(rep.lengths[g].sum()))
        rows = slice(int(offs[g]), int(offs[g + 1]))
        f = (xr[rows].astype(np.float64) @ Lr - x0.cpu().numpy()[rows].astype(np.float64) @ L) @ np.linalg.inv(Lr)
        worst = max(worst, float(np.abs(f - np.rint(f)).max()))
    print(f"natoms {natoms}: largest residual {worst:.3e} fractional, bound {FRAC_BOUND:.3e}")
    assert worst <= FRAC_BOUND


def test_a_crystal_alone_gives_the_bytes_it_gives_in_the_batch(batch65, plan65):
    idx, x, lat = batch65
    rc, out = run_raw(plan65, lat, out=torch.full((65 * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV))
    assert rc == 0, _lib.load().chm_last_error()
    rc, again = run_raw(plan65, lat)
    assert rc == 0
    whole = out.cpu().numpy().reshape(65, RECORD_BYTES)
    np.testing.assert_array_equal(whole, again.cpu().numpy().reshape(65, RECORD_BYTES))  # (also the padding)
    one = CellPlan([1], DEV)
    for g in (0, 1, 2, 17, 64):
        rc, alone = run_raw(one, lat[g:g + 1].contiguous())
        assert rc == 0
        np.testing.assert_array_equal(alone.cpu().numpy(), whole[g])


def test_graph_replay_and_eager_are_byte_identical(batch65, plan65):
    idx, x, lat = batch65
    rq = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    rc, rec = run_raw(plan65, lat, rq)
    assert rc == 0, _lib.load().chm_last_error()
    ex, el = torch.empty_like(x), torch.empty_like(lat)
    assert apply_raw(plan65, rec, x, lat, ex, el) == 0, _lib.load().chm_last_error()
    eager = [t.cpu().numpy().copy() for t in (rec, ex, el)]
    out, gx, gl = torch.zeros_like(rec), torch.zeros_like(x), torch.zeros_like(lat)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc, _ = run_raw(plan65, lat, rq, out=out)
            assert rc == 0
            assert apply_raw(plan65, out, x, lat, gx, gl) == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(0x5C)
        gx.fill_(-1.0)
        gl.fill_(-1.0)
        g.replay()
        for got, want in zip((out, gx, gl), eager):
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))
    assert np.array_equal(CellReport(eager[0]).mismatch, CellReport(eager[0]).code != 6)


def test_run_and_apply_refuse_bad_arguments(batch65, plan65):
    idx, x, lat = batch65
    lib = _lib.load()
    B = 65
    out = torch.full((B * RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    rq = torch.zeros(B, dtype=torch.int32, device=DEV)
    for kw, name in [({"n_l": 9 * B - 9}, b"lattices"), ({"n_o": 128 * B - 128}, b"out"), ({"n_o": 128 * B + 16}, b"out"),
                     ({"n_r": B - 1}, b"require"), ({"n_r": 0}, b"require"), ({"n_r": 2}, b"require"),
                     ({"symprec": 0.0}, b"symprec"), ({"symprec": 1.5}, b"symprec"),
                     ({"symprec": float("nan")}, b"symprec"), ({"angle_tolerance": -1.0}, b"angle_tolerance"),
                     ({"angle_tolerance": 30.5}, b"angle_tolerance")]:
        rc, _ = run_raw(plan65, lat, rq, out=out, **kw)
        assert rc == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    rc, _ = run_raw(plan65, lat, None, out=out, n_r=1)
    assert rc == -1 and b"require" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())  # nothing was enqueued
    rc, rec = run_raw(plan65, lat, rq[:1])
    assert rc == 0, lib.chm_last_error()
    xo, lo = torch.full_like(x, -7.0), torch.full_like(lat, -7.0)
    for kw, name in [({"n_rec": 128 * B - 128}, b"records"), ({"n_x": 3 * B - 3}, b"frac"), ({"n_l": 9}, b"lattices"),
                     ({"n_xo": 3 * B + 3}, b"frac_out"), ({"n_lo": 9 * B - 9}, b"lattices_out")]:
        assert apply_raw(plan65, rec, x, lat, xo, lo, **kw) == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    assert apply_raw(plan65, rec, x, lat, x, lo) == -1 and b"in place" in lib.chm_last_error()
    assert apply_raw(plan65, rec, x, lat, xo, lat) == -1 and b"in place" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert bool((xo == -7.0).all()) and bool((lo == -7.0).all())  # nothing was enqueued
    assert apply_raw(plan65, rec, x, lat, xo, lo) == 0, lib.chm_last_error()
    torch.cuda.synchronize()


def test_torch_op_returns_the_ctypes_bytes(batch65, plan65):
    from chemeleon_amd import ops
    chem = ops.load()
    idx, x, lat = batch65
    nat = [1] * 65
    for rq in (None, torch.full((1,), 3, dtype=torch.int32, device=DEV)):
        rc, raw = run_raw(plan65, lat, rq)
        assert rc == 0
        xo, lo = torch.empty_like(x), torch.empty_like(lat)
        assert apply_raw(plan65, raw, x, lat, xo, lo) == 0
        rec = raw.cpu().numpy().reshape(65, RECORD_BYTES)
        f, i, xr, lr = chem.cell(x, lat, nat, rq, C.SYMPREC, C.ANGLE_TOLERANCE)
        assert f.shape == (65, 8) and f.dtype == torch.float32 and i.shape == (65, 18) and i.dtype == torch.int32
        np.testing.assert_array_equal(f.cpu().numpy().view(np.uint8), rec[:, :32])
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint8), rec[:, 32:104])
        assert torch.equal(xr.view(torch.int32), xo.view(torch.int32))  # (bits: the NaN cell is copied as it is)
        assert torch.equal(lr.view(torch.int32), lo.view(torch.int32))
    with pytest.raises(RuntimeError, match="shape"):
        chem.cell(x[:-1], lat, nat, None, 0.1, 10.0)
    with pytest.raises(RuntimeError, match="require"):
        chem.cell(x, lat, nat, torch.zeros(2, dtype=torch.int32, device=DEV), 0.1, 10.0)
    with pytest.raises(RuntimeError, match="symprec"):
        chem.cell(x, lat, nat, None, 2.0, 10.0)
    with pytest.raises(RuntimeError, match="HIP device only"):
        chem.cell(x, lat.cpu(), nat, None, 0.1, 10.0)


# --------------------------------------------------------------------------- Chemeleon.sample(cell=...)
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


def test_sample_reports_every_structure(model100, final):
    kw, natoms, a, x, lat, every = final
    want = cell_states(natoms, a, x, lat)
    atoms = model100.sample(None, 6, 4, cell=Cell(), **kw)
    rep = model100.last_cell
    np.testing.assert_array_equal(rep.records, want.records)
    assert len(atoms) == 4 and [at.info["cell"]["index"] for at in atoms] == [0, 1, 2, 3]
    for g, at in enumerate(atoms):
        same_structure(at, every[g])
        assert at.info["cell"]["system"] == (str(rep.system[g]) or None) and not at.info["cell"]["reduced"]
        assert at.info["cell"]["n_ops"] == int(rep.n_ops[g])


def test_sample_returns_only_the_required_system(model100, final):
    kw, natoms, a, x, lat, every = final
    free = cell_states(natoms, a, x, lat)
    absent = next(s for s in C.SYSTEMS if s not in set(free.system.tolist()))
    for name in sorted(set(free.system.tolist()) - {""}) + [absent]:
        atoms = model100.sample(None, 6, 4, cell=Cell(require=name), **kw)
        keep = np.flatnonzero(free.system == name).tolist()
        assert [at.info["cell"]["index"] for at in atoms] == keep, name  # (for `absent`: none, an empty list)
        assert np.array_equal(model100.last_cell.mismatch, free.system != name)
        for at, g in zip(atoms, keep):
            same_structure(at, every[g])
            assert at.info["cell"]["system"] == name and at.info["cell"]["valid"]


def test_sample_returns_reduced_cells(model100, final):
    kw, natoms, a, x, lat, every = final
    xr, latr, want = reduce_states(natoms, a, x, lat)
    atoms = model100.sample(None, 6, 4, cell=Cell(reduce=True), **kw)
    np.testing.assert_array_equal(model100.last_cell.records, want.records)
    assert len(atoms) == 4
    for g, at in enumerate(atoms):
        assert at.info["cell"]["reduced"]
        np.testing.assert_array_equal(np.asarray(at.cell, dtype=np.float32), latr[g].cpu().numpy())
        np.testing.assert_allclose(np.asarray(at.get_scaled_positions()), xr[6 * g:6 * g + 6].cpu().numpy(), rtol=0,
                                   atol=1e-6)  # (exact with the built-in Atoms; ase recomputes them)
        np.testing.assert_array_equal(np.asarray(at.numbers), np.asarray(every[g].numbers))
        np.testing.assert_allclose(np.linalg.norm(np.asarray(at.cell, dtype=np.float64), axis=1),
                                   want.lengths[g], rtol=0, atol=16 * 2.0 ** -24 * float(want.lengths[g].sum()))


def test_sample_runs_screen_then_cell_then_dedup(model100, final):
    kw, natoms, a, x, lat, every = final
    free = screen_states(natoms, a, x, lat, Screen(max_length=1e6, min_distance=1e-6))
    d = float(np.sort(free.dmin)[1])  # the closest-packed sample fails the screen
    screen = Screen(max_length=1e6, min_distance=d)
    cells = cell_states(natoms, a, x, lat)
    name = next(str(s) for s in cells.system[::-1] if s)
    atoms = model100.sample(None, 6, 4, screen=screen, cell=Cell(require=name), dedup=Dedup(), **kw)
    srep, crep, drep = model100.last_screen, model100.last_cell, model100.last_dedup
    np.testing.assert_array_equal(srep.records, screen_states(natoms, a, x, lat, screen).records)
    failed = ~srep.valid | (cells.system != name)
    assert np.array_equal(crep.mismatch, cells.system != name) and 0 < failed.sum() < 4
    want = dedup_states(natoms, a, x, lat, Dedup(), failed)
    np.testing.assert_array_equal(drep.group, want.group)
    assert np.all(drep.group[failed] == -1)  # the failures of both take no part in the grouping
    keep = np.flatnonzero(want.representative).tolist()
    assert [at.info["dedup"]["index"] for at in atoms] == keep and keep
    for at, g in zip(atoms, keep):
        same_structure(at, every[g])
        assert at.info["screen"]["valid"] and at.info["cell"]["system"] == name and at.info["cell"]["index"] == g


def test_without_the_keyword_nothing_changes(model100, final):
    """What one process can show: without cell= no cell plan is created, last_cell stays unset, no structure gets
    info["cell"], and sample() returns the structures of the final state that sample_states gives. It cannot show
    bit-identity with a build that lacks the module (chemeleon_amd imports it always); that evidence is the dump of
    bench.py's final state from this build and from its parent, compared in profiles/r13/cell/."""
    from chemeleon_amd import cell as cell_module
    kw, natoms, a, x, lat, every = final
    plans = len(cell_module._plans)
    model100.last_cell = None
    atoms = model100.sample(None, 6, 4, **kw)
    assert model100.last_cell is None and len(cell_module._plans) == plans
    assert len(atoms) == 4
    for at, other in zip(atoms, every):
        same_structure(at, other)
        assert "cell" not in (getattr(at, "info", None) or {})


def test_stream_with_cell_raises(model100):
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, stream=True, cell=Cell())
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, return_trajectory=True, cell=Cell())
