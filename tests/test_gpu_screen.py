"""Screening on the device (csrc/screen.hip, chm_screen_*, chemeleon_amd.screening) against the float64
restatement of tests/screen_cases.py: the records of one ragged batch of boundary cases, the argument checks and
graph capture of chm_screen_run, the torch op, and Chemeleon.sample(screen=...).

Tolerances (tests/screen_cases.py: gate): lengths and dmin within 16 * 2^-24 * (a + b + c) absolute; the volume
within 16 * 2^-24 * a * b * c (a float32 cannot hold a volume of thousands of cubic Angstrom to within the
length gate: at 60.5 x 5 x 5 its half-ulp alone is 6e-5, the length gate 6.7e-5; the volume's own scale is
a * b * c); angles within 1e-3 degrees; formula units and flags exact."""

import ctypes
import math

import numpy as np
import pytest
import torch

from chemeleon_amd import Screen, _lib, screen_states
from chemeleon_amd.config import default_config
from chemeleon_amd.screening import RECORD_BYTES, ScreenPlan, ScreenReport
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from tests import screen_cases as S

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


@pytest.fixture(scope="module")
def state():
    a, x, lat = S.batch_arrays()
    return torch.from_numpy(a).to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(lat).to(DEV)


@pytest.fixture(scope="module")
def plan():
    return ScreenPlan(S.natoms(), DEV)


def run_raw(plan, a, x, lat, target=None, out=None, **n):
    """chm_screen_run with every count overridable -> (rc, out)."""
    B = len(plan.natoms)
    if out is None:
        out = torch.zeros(B * RECORD_BYTES, dtype=torch.uint8, device=DEV)
    rc = _lib.load().chm_screen_run(
        plan.handle, _lib.ptr(a), n.get("n_a", a.numel()), _lib.ptr(x), n.get("n_x", x.numel()), _lib.ptr(lat),
        n.get("n_l", lat.numel()), _lib.ptr(target), n.get("n_t", 0 if target is None else target.numel()),
        n.get("max_length", S.MAX_LENGTH), n.get("min_distance", S.MIN_DISTANCE), _lib.ptr(out),
        n.get("n_o", out.numel()), _lib.stream_handle())
    return rc, out


@pytest.mark.parametrize("mode", S.TARGET_MODES)
def test_records_match_float64(state, mode):
    a, x, lat = state
    rep = screen_states(S.natoms(), a, x, lat, Screen(S.MAX_LENGTH, S.MIN_DISTANCE, S.composition_for(mode)))
    ref = S.reference(mode)
    assert len(rep) == len(ref)
    for g, (c, r) in enumerate(zip(S.cases(), ref)):
        gate, name = S.gate(r["lengths"]), r["name"]
        print(f"{name}: lengths {np.abs(rep.lengths[g] - r['lengths']).max() / gate:.3f} gate, "
              f"volume {abs(rep.volume[g] - r['volume']) / (16 * 2.0 ** -24 * np.prod(r['lengths'])):.3f} gate, "
              f"angles {np.abs(rep.angles[g] - r['angles']).max():.2e} deg, dmin {rep.dmin[g]!r} ref {r['dmin']!r} "
              f"pair {rep.pair[g].tolist()} flags {rep.flags[g]} ref {r['flags']}")
        np.testing.assert_allclose(rep.lengths[g], r["lengths"], rtol=0, atol=gate, err_msg=name)
        assert abs(float(rep.volume[g]) - r["volume"]) <= 16 * 2.0 ** -24 * float(np.prod(r["lengths"])), name
        np.testing.assert_allclose(rep.angles[g], r["angles"], rtol=0, atol=1e-3, err_msg=name)
        assert rep.formula_units[g] == r["formula_units"], name
        assert rep.flags[g] == r["flags"], name
        assert bool(rep.valid[g]) == (r["flags"] == 0), name
        n = len(c["types"])
        i, j = (int(v) for v in rep.pair[g])
        if n == 1:
            assert math.isinf(rep.dmin[g]) and rep.dmin[g] > 0 and (i, j) == (-1, -1), name
            continue
        assert 0 <= i < j < n, name
        if c["compare_dmin"]:
            assert abs(float(rep.dmin[g]) - r["dmin"]) <= gate, (name, float(rep.dmin[g]), r["dmin"])
            # the pair by its own distance, not by index: symmetric structures tie
            assert abs(S.pair_distance_f64(c["lattice"], c["frac"], i, j) - r["dmin"]) <= gate, name


def test_one_atom_crystals(state):
    nat = [1, 1, 1]
    a = torch.tensor([22, 0, 500], device=DEV)
    x = torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0], [0.999, 0.5, 0.5]], device=DEV)
    lat = torch.from_numpy(np.stack([S.cell_from_parameters(4, 5, 6, 80, 95, 100, 1)] * 3)).to(DEV)
    rep = screen_states(nat, a, x, lat)
    assert np.all(np.isposinf(rep.dmin)) and np.all(rep.pair == -1)
    assert rep.flags.tolist() == [0, 0, 0] and rep.formula_units.tolist() == [1, 1, 1]
    rep = screen_states(nat, a, x, lat, Screen(composition="Ti"))
    assert rep.flags.tolist() == [0, S.COMPOSITION, S.COMPOSITION]  # (X and the clamped class 500 are no Ti)


def test_graph_replay_and_eager_are_byte_identical(plan, state):
    a, x, lat = state
    tg = torch.from_numpy(Screen(composition=S.composition_for("per_crystal")).target).to(DEV)
    rc, e1 = run_raw(plan, a, x, lat, tg, out=torch.full((len(S.natoms()) * 64,), 0xAB, dtype=torch.uint8, device=DEV))
    assert rc == 0, _lib.load().chm_last_error()
    rc, e2 = run_raw(plan, a, x, lat, tg)
    assert rc == 0
    eager = e1.cpu().numpy()
    np.testing.assert_array_equal(eager, e2.cpu().numpy())  # (also the padding, and the deterministic tie rule)
    out = torch.zeros_like(e1)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc, _ = run_raw(plan, a, x, lat, tg, out=out)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(0x5C)
        g.replay()
        np.testing.assert_array_equal(out.cpu().numpy(), eager)
    rep = ScreenReport(eager)
    assert rep.flags.tolist() == [r["flags"] for r in S.reference("per_crystal")]


def test_run_refuses_mis_sized_buffers(plan, state):
    a, x, lat = state
    lib = _lib.load()
    N, B = sum(S.natoms()), len(S.natoms())
    out = torch.full((B * 64,), 0xAB, dtype=torch.uint8, device=DEV)
    tg = torch.zeros(B * 104, dtype=torch.int32, device=DEV)
    for kw, name in [({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"), ({"n_l": 9 * B - 9}, b"lattices"),
                     ({"n_o": 64 * B - 64}, b"out"), ({"n_o": 64 * B + 16}, b"out"), ({"n_t": 103}, b"target"),
                     ({"n_t": 104 * (B - 1)}, b"target"), ({"n_t": 0}, b"target"), ({"max_length": 0.0}, b"max_length"),
                     ({"min_distance": -1.0}, b"min_distance")]:
        rc, _ = run_raw(plan, a, x, lat, tg, out=out, **kw)
        assert rc == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    rc, _ = run_raw(plan, a, x, lat, None, out=out, n_t=104)
    assert rc == -1 and b"target" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())  # nothing was enqueued
    rc, _ = run_raw(plan, a, x, lat, tg[:104], out=out)
    assert rc == 0, lib.chm_last_error()
    torch.cuda.synchronize()


def test_torch_op_returns_the_ctypes_bytes(plan, state):
    from chemeleon_amd import ops
    chem = ops.load()
    a, x, lat = state
    B = len(S.natoms())
    for mode in S.TARGET_MODES:
        t = Screen(composition=S.composition_for(mode)).target
        tg = None if t is None else torch.from_numpy(t).to(DEV)
        rc, raw = run_raw(plan, a, x, lat, None if tg is None else tg.reshape(-1))
        assert rc == 0
        rec = raw.cpu().numpy().reshape(B, 64)
        f, i = chem.screen(a, x, lat, S.natoms(), tg, S.MAX_LENGTH, S.MIN_DISTANCE)
        assert f.shape == (B, 8) and f.dtype == torch.float32 and i.shape == (B, 4) and i.dtype == torch.int32
        np.testing.assert_array_equal(f.cpu().numpy().view(np.uint8), rec[:, :32])
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint8), rec[:, 32:48])
    with pytest.raises(RuntimeError, match="shape"):
        chem.screen(a[:-1], x, lat, S.natoms(), None, 60.0, 0.5)
    with pytest.raises(RuntimeError, match="target"):
        chem.screen(a, x, lat, S.natoms(), torch.zeros(103, dtype=torch.int32, device=DEV), 60.0, 0.5)
    with pytest.raises(RuntimeError, match="HIP device only"):
        chem.screen(a, x, lat.cpu(), S.natoms(), None, 60.0, 0.5)


# --------------------------------------------------------------------------- Chemeleon.sample(screen=...)
@pytest.fixture(scope="module")
def model100():
    from chemeleon_amd import Chemeleon
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    return m.to(DEV).eval()


def test_sample_returns_exactly_the_passing_structures(model100):
    cond, null = synthetic_text_embeds(512)
    kw = dict(noise="philox", seed=4, text_embeds=cond, null_text_embeds=null)
    natoms = [6] * 8
    last = None
    for last in model100.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw):
        pass
    _, a, x, lat = last
    a, x, lat = a.clone(), x.clone(), lat.clone()
    free = screen_states(natoms, a, x, lat, Screen(max_length=1e6, min_distance=1e-6))
    assert np.all(np.isfinite(free.dmin))
    d = float(np.median(free.dmin))  # between the 4th and the 5th: both outcomes occur
    rep = screen_states(natoms, a, x, lat, Screen(max_length=1e6, min_distance=d))
    want = free.dmin >= np.float32(d)
    assert 0 < want.sum() < 8
    np.testing.assert_array_equal(rep.valid, want & (free.flags == 0))
    # the same run through sample(): the passing structures, in order, each with its record
    atoms = model100.sample(None, 6, 8, screen=Screen(max_length=1e6, min_distance=d), **kw)
    report = model100.last_screen
    np.testing.assert_array_equal(report.records, rep.records)
    keep = np.flatnonzero(report.valid).tolist()
    assert [at.info["screen"]["index"] for at in atoms] == keep and 0 < len(keep) < 8
    from chemeleon_amd.modules.schema import step_to_atoms
    every = step_to_atoms(a, x, lat, natoms)
    for at, g in zip(atoms, keep):
        np.testing.assert_array_equal(np.asarray(at.numbers), np.asarray(every[g].numbers))
        np.testing.assert_array_equal(at.get_scaled_positions(), every[g].get_scaled_positions())
        np.testing.assert_array_equal(np.asarray(at.cell), np.asarray(every[g].cell))
        assert at.info["screen"]["valid"] and at.info["screen"]["dmin"] == float(report.dmin[g])


def test_sample_with_ase_atoms(model100):
    pytest.importorskip("ase")
    cond, null = synthetic_text_embeds(512)
    atoms = model100.sample(None, 6, 8, noise="philox", seed=4, text_embeds=cond, null_text_embeds=null,
                            screen=Screen(max_length=1e6, min_distance=1e-6))
    assert len(atoms) == int(model100.last_screen.valid.sum())
    assert all("screen" in at.info for at in atoms)


def test_stream_with_screen_raises(model100):
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, stream=True, screen=Screen())
    with pytest.raises(ValueError, match="finished structures"):
        model100.sample(None, 6, 2, return_trajectory=True, screen=Screen())
