"""Screening without a GPU: Screen's validation, the argument checks of chm_screen_* that run before the device
is touched, and the conditions the shared fixtures (tests/screen_cases.py) must keep for the GPU tests to mean
what they say."""

import ctypes
import math

import numpy as np
import pytest
import torch

from chemeleon_amd import Screen, ScreenReport, _lib, screen_states
from chemeleon_amd.screening import reduced_counts
from tests import screen_cases as S


# ------------------------------------------------------------------------------------------ Screen
def test_screen_defaults_and_targets():
    s = Screen()
    assert (s.max_length, s.min_distance, s.target) == (60.0, 0.5, None)
    t = Screen(composition="Ti4O8").target
    assert t.dtype == np.int32 and t.shape == (104,) and t[22] == 1 and t[8] == 2 and t.sum() == 3
    np.testing.assert_array_equal(reduced_counts("SrTiO3"), S.reduced_target("SrTiO3"))
    per = Screen(composition=["TiO2", "Ti3O5"])
    assert per.target.shape == (2, 104) and per.target[1, 22] == 3 and per.target[1, 8] == 5
    assert per.target_for(2) is per.target


@pytest.mark.parametrize("kw", [dict(max_length=0.0), dict(max_length=-1.0), dict(min_distance=0.0),
                                dict(min_distance=float("nan")), dict(max_length=float("inf")),
                                dict(composition="Xx2O"), dict(composition="X2O"), dict(composition="tio2"),
                                dict(composition=["TiO2", "Qq"]), dict(composition=[])])
def test_screen_refuses_bad_arguments(kw):
    with pytest.raises(ValueError):
        Screen(**kw)


def test_wrong_list_length_and_cpu_tensors_are_refused_before_a_device_is_touched():
    a, x, lat = torch.zeros(5, dtype=torch.long), torch.zeros(5, 3), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="3 formulas"):
        screen_states([2, 3], a, x, lat, Screen(composition=["TiO2"] * 3))
    with pytest.raises(ValueError, match="shapes"):
        screen_states([2, 2], a, x, lat)
    with pytest.raises(RuntimeError, match="HIP device only"):
        screen_states([2, 3], a, x, lat)


def test_sample_refuses_screen_with_streaming():
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    cfg = default_config()
    cfg["timesteps"] = 10
    m = Chemeleon(cfg)
    for kw in (dict(stream=True), dict(return_trajectory=True)):
        with pytest.raises(ValueError, match="finished structures"):
            m.sample(None, 4, 2, screen=Screen(), **kw)
    with pytest.raises(ValueError, match="3 formulas"):
        m.sample(None, 4, 2, screen=Screen(composition=["TiO2"] * 3))


def test_report_unpacks_the_record_layout():
    rec = np.zeros((2, 64), dtype=np.uint8)
    rec.view(np.float32)[:, :8] = np.arange(16, dtype=np.float32).reshape(2, 8)
    rec.view(np.int32)[:, 8:12] = [[3, 7, 4, 0], [-1, -1, 1, 6]]
    r = ScreenReport(rec)
    np.testing.assert_array_equal(r.lengths, [[0, 1, 2], [8, 9, 10]])
    np.testing.assert_array_equal(r.angles, [[3, 4, 5], [11, 12, 13]])
    np.testing.assert_array_equal(r.volume, [6, 14])
    np.testing.assert_array_equal(r.dmin, [7, 15])
    np.testing.assert_array_equal(r.pair, [[3, 7], [-1, -1]])
    np.testing.assert_array_equal(r.formula_units, [4, 1])
    np.testing.assert_array_equal(r.valid, [True, False])
    assert r.record(1)["failed"] == ["too_close", "composition"] and r.record(0)["valid"]


# ------------------------------------------------------------------------------------------ C entry points
def test_entry_points_refuse_null_and_bad_arguments_without_gpu():
    lib = _lib.load()
    out = ctypes.c_void_p()
    nat = (ctypes.c_int32 * 3)(1, 5, 70)
    assert lib.chm_screen_create(None, 3, ctypes.byref(out)) == -1 and b"natoms" in lib.chm_last_error()
    assert lib.chm_screen_create(nat, 0, ctypes.byref(out)) == -1 and b"num_graphs" in lib.chm_last_error()
    assert lib.chm_screen_create(nat, 3, None) == -1 and b"out" in lib.chm_last_error()
    bad = (ctypes.c_int32 * 3)(1, 0, 70)
    assert lib.chm_screen_create(bad, 3, ctypes.byref(out)) == -1 and b"natoms[1]" in lib.chm_last_error()
    assert not out.value
    x = ctypes.c_void_p(0x10000)  # (never dereferenced: the NULL plan is refused before anything else)
    assert lib.chm_screen_run(None, x, 1, x, 3, x, 9, None, 0, 60.0, 0.5, x, 64, None) == -1
    assert b"plan" in lib.chm_last_error()
    lib.chm_screen_destroy(None)


# ------------------------------------------------------------------------------------------ the fixtures
def test_batch_covers_the_sizes_and_cells_the_kernel_branches_on():
    nat = S.natoms()
    for n in (1, 2, 64, 65, 256, 257, 300):
        assert n in nat
    ref = {r["name"]: r for r in S.reference("none")}
    # the triclinic cells span angles of 20 to 160 degrees (the skewed cells below are sharper still: 8 degrees)
    ang = np.concatenate([r["angles"] for r in ref.values() if "triclinic" in r["name"] or "deg" in r["name"]])
    assert ang.min() >= 19.5 and ang.max() <= 160.5 and ang.min() < 21 and ang.max() > 159
    assert min(r["angles"].min() for r in ref.values() if r["name"].startswith("skew")) > 8
    # image ranges 1, 2, 3 and beyond the cap; where it is 2 or 3 the 27 images alone give a wrong answer
    assert math.floor(ref["skew_R1"]["ranges"].max()) == 1
    for name, R in (("skew_R2", 2), ("skew_R2_rotated", 2), ("skew_R3", 3)):
        assert math.floor(ref[name]["ranges"].max()) == R, name
        assert ref[name]["d27"] - ref[name]["dmin"] > 1000 * S.gate(ref[name]["lengths"]), name
        assert ref[name]["flags"] == 0
    assert ref["beyond_cap"]["ranges"].max() > S.MAX_RANGE + 2 and ref["beyond_cap"]["flags"] == S.DEGENERATE
    assert ref["zero_volume"]["volume"] == 0 and ref["zero_volume"]["flags"] == S.DEGENERATE
    assert ref["long_edge"]["flags"] == S.TOO_LONG and ref["long_edge"]["lengths"].max() == 60.5
    assert ref["coincident"]["dmin"] == 0 and ref["coincident"]["flags"] & S.TOO_CLOSE
    assert ref["wrap"]["dmin"] < 1e-5  # (the unwrapped difference would be 4 A)
    assert ref["one_atom"]["dmin"] == math.inf
    # no range sits at the cap's threshold, where float32 could decide the flag differently
    for r in ref.values():
        assert np.all(np.abs(r["ranges"] - (S.MAX_RANGE + 1)) > 0.05), r["name"]


def test_composition_cases():
    shared = {r["name"]: r for r in S.reference("shared")}
    per = {r["name"]: r for r in S.reference("per_crystal")}
    assert (shared["Ti4O8"]["formula_units"], shared["Ti2O4"]["formula_units"]) == (4, 2)
    for name in ("Ti4O8", "Ti2O4", "n300_triclinic"):
        assert not shared[name]["flags"] & S.COMPOSITION
    for name in ("Ti3O5", "class_104", "one_atom", "Sr2Ti2O6_own_target"):
        assert shared[name]["flags"] & S.COMPOSITION
    for name in ("Ti3O5_own_target", "Sr2Ti2O6_own_target", "one_atom", "Ti4O8"):
        assert not per[name]["flags"] & S.COMPOSITION
    assert per["class_104"]["flags"] & S.COMPOSITION and per["Ti3O5"]["flags"] & S.COMPOSITION
    assert all(not r["flags"] & S.COMPOSITION for r in S.reference("none"))
    # both outcomes of every other criterion occur too
    flags = [r["flags"] for r in S.reference("none")]
    assert any(f == 0 for f in flags) and any(f & S.TOO_CLOSE for f in flags) and any(f & S.TOO_LONG for f in flags)


def test_float32_two_pass_search_stays_inside_the_gate():
    """The method (27 images, then the range from the plane spacings) in the kernel's number format against the
    float64 brute force, on every uncapped case; and every case is further than the gate from the thresholds,
    so no flag of the GPU test hangs on rounding."""
    for c, r in zip(S.cases(), S.reference("none")):
        g = S.gate(r["lengths"])
        lens, vol, dmin, capped = S.two_pass_f32(c["lattice"], c["frac"])
        assert capped == bool(r["flags"] & S.DEGENERATE), r["name"]
        np.testing.assert_allclose(lens, r["lengths"], rtol=0, atol=g, err_msg=r["name"])
        assert abs(float(vol) - r["volume"]) <= 16 * 2.0 ** -24 * float(np.prod(r["lengths"])), r["name"]
        if c["compare_dmin"]:
            assert not capped
            if math.isinf(r["dmin"]):
                assert math.isinf(dmin)
            else:
                assert abs(dmin - r["dmin"]) <= g, (r["name"], dmin, r["dmin"])
        else:
            assert capped, r["name"]
        if math.isfinite(r["dmin"]):
            assert abs(r["dmin"] - S.MIN_DISTANCE) > 10 * g, r["name"]
            assert abs(dmin - S.MIN_DISTANCE) > 10 * g, r["name"]  # (also the capped search's value)
        assert abs(r["lengths"].max() - S.MAX_LENGTH) > 10 * g, r["name"]
