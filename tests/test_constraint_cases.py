"""Constrained sampling on the CPU: the reference of tests/constraint_cases.py against the oracle's own step, the
properties the GPU tests (tests/test_gpu_constraint.py) lean on, Constraint's host validation and the ABI's
device-free refusals."""

import ctypes

import pytest
import torch

from chemeleon_amd import Constraint, _lib
from oracle import chemeleon_oracle as O

from . import constraint_cases as C


@pytest.fixture(scope="module")
def ref():
    return C.oracle_model()


@pytest.fixture(scope="module")
def tables(ref):
    return C.tables_of(ref)


def _graph_index(nat):
    n = torch.tensor(nat)
    return n, torch.arange(len(nat)).repeat_interleave(n)


@pytest.mark.parametrize("t", C.STEP_TS)
def test_no_mask_is_the_oracle_step(ref, tables, t):
    nat = [3, 5, 8, 1]
    (a, x, l), nz, con, cnz = C.step_inputs(nat, t)
    free = Constraint(nat, con.atom_types, torch.zeros_like(con.type_mask), con.frac_coords,
                      torch.zeros_like(con.frac_mask), con.lattices, torch.zeros_like(con.lattice_mask))
    n, n2g = _graph_index(nat)
    cond, null = C.conditioning(len(nat))
    want = ref.step(t, a, x, l, n, n2g, cond, null, nz)
    got = C.constrained_step(ref, t, a, x, l, n, n2g, cond, null, nz, free, cnz, tables)
    for k in range(3):
        assert torch.equal(got[k], want[k]), f"t={t} field {k}"


def test_level_zero_returns_the_known_values(tables):
    for N in C.KERNEL_NODES:
        nat, state, con, noise = C.kernel_inputs(N, "all", 99)
        a, x, l = C.replace(0, state, con, noise, tables)
        assert torch.equal(a, con.atom_types)
        assert torch.equal(l, con.lattices * O.LATTICE_MASK)
        assert torch.equal(x, con.frac_coords % 1.0)
        assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_unmasked_entries_are_untouched(tables):
    nat, state, con, noise = C.kernel_inputs(257, "alt", 5)
    out = C.replace(50, state, con, noise, tables)
    assert torch.equal(out[0][~con.type_mask], state[0][~con.type_mask])
    assert torch.equal(out[1][~con.frac_mask], state[1][~con.frac_mask])
    assert torch.equal(out[2][~con.lattice_mask], state[2][~con.lattice_mask])
    only_x = C.replace(50, state, con, noise, tables, what=4)
    assert torch.equal(only_x[0], state[0]) and torch.equal(only_x[2], state[2])
    assert torch.equal(only_x[1], out[1])


def test_stage_order_is_visible_at_the_gpu_gate(ref, tables, t=50):
    """The GPU step test can tell the stage order apart: at t = 50, with stage 1 moved behind the corrector, the
    free atoms' coordinates of the crystals with held types move by at least 10 x the gate it applies to them
    (measured: 1.9e-2 and 4.7e-2). The other steps of that test cannot show the order and check the rest: at
    level 99 the forward-noised types are the absorbing class, as the step's own samples (the difference is
    exactly 0), and at t <= 2 the corrector's step, step_lr (sigma_t / sigma_begin)^2 ~ 1e-5, is below the gate."""
    nat = [3, 5, 8, 1]
    (a, x, l), nz, con, cnz = C.step_inputs(nat, t)
    n, n2g = _graph_index(nat)
    cond, null = C.conditioning(len(nat))
    good = C.constrained_step(ref, t, a, x, l, n, n2g, cond, null, nz, con, cnz, tables)
    late = C.constrained_step(ref, t, a, x, l, n, n2g, cond, null, nz, con, cnz, tables, stage1_late=True)
    for g in (0, 2):
        rows = (n2g == g) & ~con.frac_mask
        d = (good[1][rows] - late[1][rows]).abs()
        d = torch.minimum(d, 1 - d)
        print(f"t={t} crystal {g}: free coordinates move by {float(d.max()):.3e}")
        assert float(d.max()) >= 10 * C.STEP_GATE


def test_type_noise_has_no_near_ties(tables):
    """Every constrained node of the GPU type comparisons has a float64 top-2 gap of its Gumbel scores >= 1e-3
    (fp32 log differences between device and host are ~1e-6), so those comparisons need no tie exemption."""
    worst = float("inf")
    for N, mask, level, seed in C.kernel_cases():
        if level == 0 or mask == "none":
            continue
        _nat, _state, con, noise = C.kernel_inputs(N, mask, seed)
        worst = min(worst, float(C.type_score_gaps(level, con, noise[0], tables).min()))
    for N in C.KERNEL_NODES:  # (the device-t case of the kernel test, level 50)
        for mask in ("all", "alt"):
            _nat, _state, con, noise = C.kernel_inputs(N, mask, C.KERNEL_SEED + 1000)
            worst = min(worst, float(C.type_score_gaps(50, con, noise[0], tables).min()))
    for nat in C.STEP_NATOMS:
        for t in C.STEP_TS:
            if t == 1:
                continue
            _s, _nz, con, cnz = C.step_inputs(nat, t)
            worst = min(worst, float(C.type_score_gaps(t - 1, con, cnz[0], tables).min()))
    for N, level, seed, node_base, _gb in C.PHILOX_CASES:
        if level == 0:
            continue
        _nat, _state, con, _noise = C.kernel_inputs(N, "all", seed)
        u = C.philox_type_uniforms(seed, level + 1, node_base, N)
        worst = min(worst, float(C.type_score_gaps(level, con, u, tables).min()))
    print(f"smallest top-2 gap {worst:.3e}")
    assert worst >= 1e-3


def test_philox_host_stream_is_uniform():
    u = C.philox_uniform(7, 50, 4, torch.arange(1 << 16).numpy())
    assert u.dtype.name == "float32" and u.min() >= 0.0 and u.max() < 1.0
    assert abs(float(u.mean()) - 0.5) < 5 * (1 / 12 / (1 << 16)) ** 0.5
    assert len(set(u.tolist())) > 65000


# ------------------------------------------------------------------------------------------ Constraint
def _valid(N=5, B=2):
    return dict(atom_types=torch.arange(N), type_mask=torch.ones(N, dtype=torch.bool), frac_coords=torch.rand(N, 3),
                frac_mask=torch.zeros(N, dtype=torch.bool), lattices=torch.eye(3).repeat(B, 1, 1),
                lattice_mask=torch.ones(B, dtype=torch.bool))


@pytest.mark.parametrize("field,bad", [
    ("atom_types", torch.zeros(4, dtype=torch.long)), ("type_mask", torch.ones(6, dtype=torch.bool)),
    ("frac_coords", torch.zeros(5, 2)), ("frac_mask", torch.ones(5, 1, dtype=torch.bool)),
    ("lattices", torch.zeros(2, 9)), ("lattice_mask", torch.ones(3, dtype=torch.bool))])
def test_wrong_shapes_are_refused(field, bad):
    kw = _valid()
    Constraint.from_arrays([2, 3], **kw)
    kw[field] = bad
    with pytest.raises(ValueError, match=field):
        Constraint.from_arrays([2, 3], **kw)


def test_bad_values_are_refused():
    kw = _valid()
    kw["atom_types"] = torch.tensor([1, 2, 3, 104, 5])
    with pytest.raises(ValueError, match="104"):
        Constraint.from_arrays([2, 3], **kw)
    kw = _valid()
    kw["atom_types"] = torch.tensor([1, 2, -1, 4, 5])
    with pytest.raises(ValueError, match="atom_types"):
        Constraint.from_arrays([2, 3], **kw)
    kw = _valid()
    kw["frac_coords"][3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        Constraint.from_arrays([2, 3], **kw)
    kw = _valid()
    kw["lattices"][1, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        Constraint.from_arrays([2, 3], **kw)
    with pytest.raises(ValueError, match="mask"):
        Constraint.from_arrays([2, 3], type_mask=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError):
        Constraint.composition([2, 3], [[1, 1], [8, 8]])
    c = Constraint.from_arrays([2, 3], atom_types=torch.arange(5))
    with pytest.raises(ValueError, match="crystals"):
        c.check_batch([3, 2])


def test_from_formula():
    with pytest.raises(ValueError, match="multiple"):
        Constraint.from_formula("TiO2", 10, 4)
    with pytest.raises(ValueError):
        Constraint.from_formula("Ti O2)", 12, 2)
    with pytest.raises(ValueError, match="unknown element"):
        Constraint.from_formula("Zz2", 12, 2)
    c = Constraint.from_formula("TiO2", 12, 2)
    assert c.natoms == [12, 12] and bool(c.type_mask.all())
    assert not bool(c.frac_mask.any()) and not bool(c.lattice_mask.any())
    for g in range(2):
        z = c.atom_types[12 * g:12 * g + 12].tolist()
        assert z.count(22) == 4 and z.count(8) == 8
    assert Constraint.from_formula("Ti2O4", 3, 1).atom_types.tolist() == [22, 8, 8]  # (the reduced formula counts)


# ------------------------------------------------------------------------------------------ the ABI without a device
def test_null_batch_is_refused_by_both_entry_points():
    lib = _lib.load()
    io, con, sched = _lib.chm_step_io(), _lib.chm_constraint(), _lib.chm_schedule()
    assert lib.chm_sample_step_con(None, ctypes.byref(sched), 1, None, 2.0, ctypes.byref(io), ctypes.byref(con), 0, 0,
                                   0, None) == -1
    assert b"batch" in lib.chm_last_error()
    assert lib.chm_constrain_state(None, ctypes.byref(sched), ctypes.byref(con), 0, None, 7, ctypes.byref(io), 0, 0,
                                   0, None) == -1
    assert b"batch" in lib.chm_last_error()
