"""The crystal-system cases and their restatements on the CPU (tests/symmetry_cases.py): the float64 restatement
gives the textbook values, the float32 restatement (what the device is pinned to, tests/test_gpu_symmetry.py)
equals it on every integer field, every distance test keeps its margin, and the host side of
chemeleon_amd.symmetry (validation, report parsing, names) works without a device."""

import numpy as np
import pytest
import torch

from chemeleon_amd import CRYSTAL_SYSTEMS, Symmetry, SymmetryReport, symmetry_states
from chemeleon_amd import symmetry as sym
from chemeleon_amd.cell import SYSTEMS
from tests import symmetry_cases as S


def test_float64_restatement_gives_the_textbook_values():
    by_name = {c["name"]: r for c, r in zip(S.cases(), S.reference("float64"))}
    assert set(S.EXPECTED) <= set(by_name)  # no named base case was dropped
    for c, r in zip(S.cases(), S.reference("float64")):
        want = S.EXPECTED.get(c["family"])  # (a variant must give what its base case gives)
        if want is not None and c["name"] in (c["family"], f'{c["family"]}_v0', f'{c["family"]}_v1'):
            got = (CRYSTAL_SYSTEMS[r["system"]], r["n_pg"], r["inversion"], r["n_trans"])
            assert got == want and r["flags"] == 0 and r["halvings"] == 0, (c["name"], got, want)
            base = by_name[c["family"]]
            assert all(r[f] == base[f] for f in S.INT_FIELDS) and r["tol"] == base["tol"], c["name"]
    for name, lattice in S.EXPECTED_LATTICE.items():
        assert SYSTEMS[by_name[name]["lattice_system"]] == lattice, name
    for name, (system, n_pg, inv, n_trans, n_pivot) in S.SIZE_EXPECTED.items():
        r = by_name[name]
        assert (CRYSTAL_SYSTEMS[r["system"]], r["n_pg"], r["inversion"], r["n_trans"], r["n_pivot"]) == \
            (system, n_pg, inv, n_trans, n_pivot), name
        assert r["n_sym"] == n_pg * n_trans
    kept, lost, halved = by_name["rocksalt8_d002"], by_name["rocksalt8_d04"], by_name["one_halving"]
    assert (kept["system"], kept["n_pg"], kept["n_trans"], kept["halvings"]) == (6, 48, 4, 0)  # 0.02 A: kept
    assert lost["system"] != 6 and lost["n_pg"] < 48 and lost["lattice_system"] == 6          # 0.4 A: lost
    assert halved["halvings"] >= 1 and halved["flags"] == 0 and halved["tol"] == np.float32(0.1) / 2
    assert by_name["thin"]["flags"] == S.THIN and by_name["thin"]["system"] == -1 and by_name["thin"]["lattice_system"] == 2
    assert by_name["no_lattice"]["flags"] == S.NO_LATTICE and by_name["no_lattice"]["lattice_system"] == -1
    assert S.restate(S.cases()[0], np.float64, require=3)["flags"] == S.MISMATCH
    assert S.reference("float64", 3)[0]["flags"] == S.MISMATCH and S.reference("float64", 6)[0]["flags"] == 0
    assert sorted(len(c["types"]) for c in S.cases() if c["name"].startswith(("sc_", "simple_cubic", "cscl")))[-4:] == \
        [63, 64, 65, 256]


def test_float32_restatement_equals_float64_on_every_integer_field():
    for c, a, b in zip(S.cases(), S.reference("float64"), S.reference("float32")):
        assert all(a[f] == b[f] for f in S.INT_FIELDS), (c["name"], a, b)
        assert a["tol"] == b["tol"] and [o[0] for o in a["ops"]] == [o[0] for o in b["ops"]]


def test_every_distance_test_keeps_its_margin():
    for c, r in zip(S.cases(), S.reference("float64")):
        assert r["margin"] >= S.MARGIN and r["lattice_margin"] >= S.MARGIN, (c["name"], r["margin"], r["lattice_margin"])
    n_variants = S.VARIANTS * len(S.EXPECTED)
    assert len(S.dropped_variants()) <= 0.05 * n_variants


def test_halving_search_is_reproducible():
    assert S.find_halving() == S.HALVING


def test_symmetry_validation():
    s = Symmetry()
    assert (s.symprec, s.angle_tolerance, s.codes) == (0.1, 10.0, None) and s.codes_for(7) is None
    assert Symmetry(require="trigonal").codes.tolist() == [4] and Symmetry(require="cubic").codes_for(9).tolist() == [6]
    assert Symmetry(require=["cubic", "triclinic"]).codes_for(2).tolist() == [6, 0]
    with pytest.raises(ValueError, match="2 crystal systems"):
        Symmetry(require=["cubic", "triclinic"]).codes_for(3)
    for bad in (dict(symprec=0), dict(symprec=1.5), dict(symprec="0.1"), dict(symprec=True), dict(angle_tolerance=31),
                dict(angle_tolerance=float("nan")), dict(require="rhombohedral"), dict(require=[]), dict(require=3),
                dict(require=["cubic", None])):
        with pytest.raises(ValueError):
            Symmetry(**bad)
    with pytest.raises(ValueError, match="chemeleon_amd.Symmetry"):
        symmetry_states([1], torch.zeros(1, dtype=torch.long), torch.zeros(1, 3), torch.eye(3)[None], "cubic")
    with pytest.raises(RuntimeError, match="HIP device only"):
        symmetry_states([1], torch.zeros(1, dtype=torch.long), torch.zeros(1, 3), torch.eye(3)[None])
    with pytest.raises(ValueError, match="shapes"):
        symmetry_states([2], torch.zeros(1, dtype=torch.long), torch.zeros(1, 3), torch.eye(3)[None])


def test_names_and_flags():
    assert CRYSTAL_SYSTEMS == ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")
    assert CRYSTAL_SYSTEMS == S.CRYSTAL_SYSTEMS and SYSTEMS[4] == "rhombohedral"
    assert sym.FLAG_NAMES == {1: "ambiguous", 2: "mismatch", 4: "no_lattice", 8: "thin"}
    assert (sym.AMBIGUOUS, sym.MISMATCH, sym.NO_LATTICE, sym.THIN) == (S.AMBIGUOUS, S.MISMATCH, S.NO_LATTICE, S.THIN)
    assert sym.RECORD_BYTES == 64 and sym.MAX_OPS == S.MAX_OPS == 48
    assert np.array_equal(sym.candidate_matrix(S.IDENTITY_INDEX), np.eye(3, dtype=np.int64))
    assert np.array_equal(sym.candidate_matrix(3 ** 9 - 1 - S.IDENTITY_INDEX), -np.eye(3, dtype=np.int64))
    header = open(S.cc.__file__.replace("tests/cell_cases.py", "include/chemeleon_hip.h")).read()
    for name, value in (("CHM_SYMM_TRIGONAL", 4), ("CHM_SYMM_CUBIC", 6), ("CHM_SYMM_NO_LATTICE", 4), ("CHM_SYMM_THIN", 8),
                        ("CHM_SYMM_MAX_OPS", 48)):
        assert f"#define {name} {value}" in header


def test_report_parsing():
    i = np.zeros((2, 16), dtype=np.int32)
    i[0, :14] = [4, 6, 1, 6, 6, 3, 2, 0, 0, 0, 1, 0, 3, 5]
    i[1, :14] = [-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, S.NO_LATTICE | S.MISMATCH, 0, -1]
    i.view(np.float32)[0, 14] = 0.05
    slots = np.zeros((2, 48, 4), dtype=np.int32)
    slots[:, :, 0] = -1
    slots[0, 0, 0] = S.IDENTITY_INDEX
    slots.view(np.float32)[0, 0, 1:] = [0.25, 0.5, 0.0]
    rep = SymmetryReport(i.view(np.uint8), slots.view(np.uint8))
    assert len(rep) == 2 and rep.system.tolist() == ["trigonal", ""] and rep.lattice_system.tolist() == ["hexagonal", ""]
    assert rep.valid.tolist() == [True, False] and rep.mismatch.tolist() == [False, True]
    r = rep.record(0)
    assert (r["system"], r["n_sym"], r["n_pg"], r["orders"], r["halvings"], r["n_pivot"], r["lattice_system"]) == \
        ("trigonal", 6, 6, (3, 2, 0, 0), 1, 3, "hexagonal")
    assert r["tol"] == float(np.float32(0.05)) and r["failed"] == [] and not r["inversion"]
    assert rep.record(1)["failed"] == ["mismatch", "no_lattice"] and rep.record(1)["system"] is None
    ids, W, t = rep.operations[0]
    assert ids.tolist() == [S.IDENTITY_INDEX] and np.array_equal(W[0], np.eye(3)) and t.tolist() == [[0.25, 0.5, 0.0]]
    assert rep.operations[1][1].shape == (0, 3, 3)
