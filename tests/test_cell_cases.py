"""Lattice system and reduced cell without a GPU: the float64 restatement of tests/cell_cases.py gives the known
system for every built case and is invariant under basis changes and rotations, the margin condition that makes
the GPU test's exact comparisons well posed, Cell's validation, CellReport's unpacking, and the argument checks of
chm_cell_* that run before the device is touched."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import Cell, CellReport, _lib, cell_states, reduce_states
from chemeleon_amd.cell import RECORD_BYTES, SYSTEMS, system_code
from tests import cell_cases as C


# ------------------------------------------------------------------------------------------ the reference
def test_candidate_set():
    W, det, tr = C.candidates()
    assert len(W) == 6960 and set(np.unique(det)) == {-1, 1} and W.min() == -1 and W.max() == 1
    assert (det == 1).sum() == 3480


def test_reference_gives_the_known_system_for_every_case():
    names = set()
    for c, r in zip(C.cases(), C.reference()):
        assert r["code"] == c["system"], (c["name"], r["counts"], r["halvings"])
        names.add(c["family"])
        if c["system"] >= 0:
            assert r["flags"] == 0 and r["counts"] in C.SIGNATURES and r["passes"] < C.MAX_PASSES, c["name"]
    for name in ("cubic", "tetragonal", "orthorhombic", "hexagonal", "rhombohedral_acute", "rhombohedral_obtuse",
                 "monoclinic", "triclinic", "fcc_primitive", "bcc_primitive", "bct_primitive", "ortho_C_primitive",
                 "ortho_F_primitive", "ortho_I_primitive", "mono_C_primitive", "near_cubic", "one_halving",
                 "zero_volume", "nan", "not_reduced"):
        assert name in names, name
    ref = {c["name"]: r for c, r in zip(C.cases(), C.reference())}
    assert ref["one_halving"]["halvings"] == 1 and ref["near_cubic"]["halvings"] == 0
    assert ref["zero_volume"]["flags"] == C.DEGENERATE and ref["nan"]["flags"] == C.NONFINITE
    # strong shears reduce in a few passes (whole multiples, not unit steps against the cap of 100)
    assert ref["cubic_shear150"]["passes"] <= 3 and np.abs(ref["cubic_shear150"]["transform"]).max() == 150
    assert ref["triclinic_shear1000"]["passes"] <= 10 and np.abs(ref["triclinic_shear1000"]["transform"]).max() == 1000
    np.testing.assert_allclose(ref["triclinic_shear1000"]["lengths"], ref["triclinic"]["lengths"], rtol=0, atol=2e-3)
    # beyond the cap of T's entries: flagged, no system, no counts, and a required system is not met
    nr = ref["not_reduced"]
    assert (nr["flags"], nr["code"], nr["counts"]) == (C.NOT_REDUCED, -1, (0, 0, 0, 0, 0))
    assert {c["name"]: r for c, r in zip(C.cases(), C.reference(1))}["not_reduced"]["flags"] == C.NOT_REDUCED | C.MISMATCH
    assert ref["cubic"]["counts"][0] == 48 and ref["triclinic"]["counts"][0] == 2
    assert sorted({r["code"] for r in C.reference()}) == [-1, 0, 1, 2, 3, 4, 5, 6]


def test_system_and_reduced_metric_are_invariant_under_basis_change_and_rotation():
    cs, ref = C.cases(), C.reference()
    base = {c["name"]: r for c, r in zip(cs, ref) if c["name"] == c["family"]}
    moved = 0
    for c, r in zip(cs, ref):
        if c["name"] == c["family"]:
            continue
        moved += 1
        b = base[c["family"]]
        assert (r["code"], r["counts"], r["halvings"]) == (b["code"], b["counts"], b["halvings"]), c["name"]
        assert np.abs(r["transform"]).max() > 1 or not np.array_equal(np.abs(r["transform"]), np.eye(3)), c["name"]
        # the moved cell is the same lattice only up to its own rounding to float32: an entry of the reduced
        # cell is a sum of three input entries (half an ulp each) times entries of T
        d = 3.0 * float(np.abs(r["transform"]).max()) * 2.0 ** -24 * float(np.abs(c["lattice"]).max())
        np.testing.assert_allclose(r["lengths"], b["lengths"], rtol=0, atol=2 * d, err_msg=c["name"])
        assert abs(r["volume"] - b["volume"]) <= 6 * d / b["lengths"].min() * b["volume"], c["name"]
        if c["tie_free"]:
            np.testing.assert_allclose(r["angles"], b["angles"], rtol=0, atol=np.degrees(8 * d / b["lengths"].min()),
                                       err_msg=c["name"])
    assert moved >= 45


def test_reduced_cells_are_reduced():
    for c, r in zip(C.cases(), C.reference()):
        if r["flags"] & (C.DEGENERATE | C.NONFINITE):
            assert np.array_equal(r["transform"], np.eye(3, dtype=np.int64))
            continue
        if r["flags"] & C.NOT_REDUCED:  # (it keeps what it has: some unimodular T)
            assert round(float(np.linalg.det(r["transform"]))) == 1
            continue
        T = r["transform"]
        assert round(float(np.linalg.det(T))) == 1, c["name"]
        np.testing.assert_allclose(T @ c["lattice"].astype(np.float64), r["lattice"], rtol=0,
                                   atol=2.0 ** -23 * float(r["lengths"].max()), err_msg=c["name"])
        ln = r["lengths"]
        assert ln[0] <= ln[1] * (1 + 1e-5) and ln[1] <= ln[2] * (1 + 1e-5), c["name"]
        assert np.all(r["angles"] > 59.99) and np.all(r["angles"] < 120.01), c["name"]


def test_margin_condition():
    """Every candidate of every case is at least 1e-3 of the tolerance away from the tolerance, at every level
    the case visits: the float32 search on the device decides every candidate as float64 does."""
    for c, r in zip(C.cases(), C.reference()):
        assert r["margin"] >= C.MARGIN, (c["name"], r["margin"])
    for req in (2, 6):  # (the required system changes only the MISMATCH bit)
        for r0, r in zip(C.reference(), C.reference(req)):
            assert r["flags"] & ~C.MISMATCH == r0["flags"] and bool(r["flags"] & C.MISMATCH) == (r["code"] != req)


def test_batches_mix_systems_and_flags():
    cs = C.cases()
    assert len(cs) >= 60
    small = [cs[k]["name"] for k in C.batch(3)]
    assert small == ["cubic", "nan", "one_halving"]
    b65 = C.batch(65)
    assert len(b65) == 65 and len(set(b65)) == 65 and len(cs) >= 65
    for name in ("zero_volume", "not_reduced", "cubic_shear150", "triclinic_shear1000", "triclinic", "near_cubic"):
        assert name in [cs[k]["name"] for k in b65], name


# ------------------------------------------------------------------------------------------ Cell, CellReport
def test_cell_defaults_and_requirements():
    c = Cell()
    assert (c.symprec, c.angle_tolerance, c.codes, c.reduce) == (0.1, 10.0, None, False)
    assert Cell(require="cubic").codes.tolist() == [6] and Cell(require="cubic").codes.dtype == np.int32
    per = Cell(require=["cubic", "triclinic"])
    assert per.codes.tolist() == [6, 0] and per.codes_for(2) is per.codes
    assert Cell(require=["hexagonal"]).codes_for(1).tolist() == [5]
    assert Cell(require="cubic").codes_for(7).tolist() == [6]
    assert [system_code(s) for s in SYSTEMS] == list(range(7)) and SYSTEMS == C.SYSTEMS
    with pytest.raises(ValueError, match="2 lattice systems"):
        per.codes_for(3)


@pytest.mark.parametrize("kw", [dict(symprec=0.0), dict(symprec=-0.1), dict(symprec=1.5), dict(symprec=float("nan")),
                                dict(symprec="0.1"), dict(angle_tolerance=0.0), dict(angle_tolerance=31.0),
                                dict(angle_tolerance=float("inf")), dict(angle_tolerance=True), dict(require="Cubic"),
                                dict(require="trigonal"), dict(require=6), dict(require=["cubic", "fcc"]),
                                dict(require=[]), dict(reduce="yes")])
def test_cell_refuses_bad_arguments(kw):
    with pytest.raises(ValueError):
        Cell(**kw)


def test_wrong_shapes_and_cpu_tensors_are_refused_before_a_device_is_touched():
    a, x, lat = torch.zeros(5, dtype=torch.long), torch.zeros(5, 3), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="3 lattice systems"):
        cell_states([2, 3], a, x, lat, Cell(require=["cubic"] * 3))
    with pytest.raises(ValueError, match="shapes"):
        cell_states([2, 2], a, x, lat)
    with pytest.raises(ValueError, match="chemeleon_amd.Cell"):
        cell_states([2, 3], a, x, lat, "cubic")
    with pytest.raises(RuntimeError, match="HIP device only"):
        cell_states([2, 3], a, x, lat)
    with pytest.raises(RuntimeError, match="HIP device only"):
        reduce_states([2, 3], None, x, lat)


def test_sample_refuses_cell_with_streaming():
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    cfg = default_config()
    cfg["timesteps"] = 10
    m = Chemeleon(cfg)
    for kw in (dict(stream=True), dict(return_trajectory=True)):
        with pytest.raises(ValueError, match="finished structures"):
            m.sample(None, 4, 2, cell=Cell(), **kw)
    with pytest.raises(ValueError, match="3 lattice systems"):
        m.sample(None, 4, 2, cell=Cell(require=["cubic"] * 3))
    with pytest.raises(ValueError, match="chemeleon_amd.Cell"):
        m.sample(None, 4, 2, cell="cubic")


def test_report_unpacks_the_record_layout():
    rec = np.zeros((2, RECORD_BYTES), dtype=np.uint8)
    rec.view(np.float32)[:, :7] = np.arange(14, dtype=np.float32).reshape(2, 7)
    i = rec.view(np.int32)
    i[0, 8:17] = [0, -1, 0, -1, 0, 0, 0, 0, -1]
    i[1, 8:17] = [1, 0, 0, 0, 1, 0, 2, 0, 1]
    i[0, 17:26] = [48, 9, 8, 6, 0, 6, 0, 0, 7]
    i[1, 17:26] = [6, 1, 0, 0, 0, -1, 4, C.AMBIGUOUS | C.MISMATCH, 3]
    r = CellReport(rec)
    assert len(r) == 2
    np.testing.assert_array_equal(r.lengths, [[0, 1, 2], [7, 8, 9]])
    np.testing.assert_array_equal(r.angles, [[3, 4, 5], [10, 11, 12]])
    np.testing.assert_array_equal(r.volume, [6, 13])
    np.testing.assert_array_equal(r.transform[1], [[1, 0, 0], [0, 1, 0], [2, 0, 1]])
    np.testing.assert_array_equal(r.n_ops, [48, 6])
    np.testing.assert_array_equal(r.orders, [[9, 8, 6, 0], [1, 0, 0, 0]])
    assert r.system.tolist() == ["cubic", ""] and r.code.tolist() == [6, -1]
    assert r.halvings.tolist() == [0, 4] and r.passes.tolist() == [7, 3]
    assert r.valid.tolist() == [True, False] and r.mismatch.tolist() == [False, True]
    d = r.record(1)
    assert d["failed"] == ["ambiguous", "mismatch"] and d["system"] is None and d["transform"][2] == (2, 0, 1)
    assert r.record(0)["system"] == "cubic" and r.record(0)["valid"] and r.record(0)["orders"] == (9, 8, 6, 0)
    i[0, 24] = C.NOT_REDUCED
    assert CellReport(rec).valid.tolist() == [False, False]  # (a cell that is not reduced is not classified)


# ------------------------------------------------------------------------------------------ C entry points
def test_entry_points_refuse_null_and_bad_arguments_without_gpu():
    lib = _lib.load()
    out = ctypes.c_void_p()
    nat = (ctypes.c_int32 * 3)(1, 5, 70)
    assert lib.chm_cell_create(None, 3, ctypes.byref(out)) == -1 and b"natoms" in lib.chm_last_error()
    assert lib.chm_cell_create(nat, 0, ctypes.byref(out)) == -1 and b"num_graphs" in lib.chm_last_error()
    assert lib.chm_cell_create(nat, 3, None) == -1 and b"out" in lib.chm_last_error()
    bad = (ctypes.c_int32 * 3)(1, 0, 70)
    assert lib.chm_cell_create(bad, 3, ctypes.byref(out)) == -1 and b"natoms[1]" in lib.chm_last_error()
    assert not out.value
    x = ctypes.c_void_p(0x10000)  # (never dereferenced: the NULL plan is refused before anything else)
    assert lib.chm_cell_run(None, x, 9, None, 0, 0.1, 10.0, x, 128, None) == -1
    assert b"plan" in lib.chm_last_error()
    assert lib.chm_cell_apply(None, x, 128, x, 3, x, 9, x, 3, x, 9, None) == -1
    assert b"plan" in lib.chm_last_error()
    lib.chm_cell_destroy(None)
