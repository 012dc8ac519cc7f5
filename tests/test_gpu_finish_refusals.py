"""The refusals of the finishing legs, in full: every chm_*_create and every chm_*_run / _apply / _fingerprint / _group
of screen, cell, symmetry, dedup, match and match-group is driven through ctypes once per refusal branch, and the
return code and the complete chm_last_error() string are compared with what the library has always said. The same
for the ValueError / RuntimeError texts of the six *_states functions, and the plan caches' identity and eviction
order. No call gets as far as a launch: every buffer is a pointer into one zeroed device allocation.

The crystal list is [1, 2] (B = 2, N = 3); match adds the references [2] (R = 1, NR = 2) and ref_of = [-1, 0]. The
pair-record counts of match-group need a plan with a pair: [2, 2] for those three cases.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd import cell as cell_module
from chemeleon_amd import dedup as dedup_module
from chemeleon_amd import match as match_module
from chemeleon_amd import match_group as match_group_module
from chemeleon_amd import screening as screen_module
from chemeleon_amd import symmetry as symmetry_module

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
ARG, UNSUPPORTED = -1, -3
NAN, INF = math.nan, math.inf
NATOMS, B, N = [1, 2], 2, 3
REFS, R, NR = [2], 1, 2
REF_OF = [-1, 0]


def i32(values):
    return (ctypes.c_int32 * len(values))(*values)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def slots():
    """slot(k): a 256-byte aligned device address, distinct per k; none is ever read or written."""
    buf = torch.zeros(64 * 256, dtype=torch.uint8, device=DEV)
    base = (buf.data_ptr() + 255) // 256 * 256

    def slot(k, offset=0):
        assert 0 <= k < 63
        return ctypes.c_void_p(base + 256 * k + offset)

    slot.keep = buf
    return slot


def refused(lib, fn, base, cases):
    """Calls fn with `base` (an ordered dict of valid arguments) changed by each case's overrides and compares
    (rc, chm_last_error()) with the case's."""
    bad = []
    for changes, code, text in cases:
        unknown = set(changes) - set(base)
        assert not unknown, unknown
        args = dict(base, **changes)
        rc = getattr(lib, fn)(*args.values())
        got = lib.chm_last_error().decode()
        if (rc, got) != (code, text):
            bad.append((fn, changes, rc, got, code, text))
    assert not bad, bad


# ---------------------------------------------------------------- plan creation
CREATE = [("screen", "screen", None), ("cell", "cell plan", None), ("symm", "symmetry plan", "the symmetry search"),
          ("dedup", "dedup plan", None), ("match_group", "match plan", "the matcher")]


@pytest.mark.parametrize("leg,plan,holder", CREATE, ids=[c[0] for c in CREATE])
def test_create_refusals(lib, leg, plan, holder):
    h = ctypes.c_void_p()
    base = dict(natoms=i32(NATOMS), count=B, out=ctypes.byref(h))
    cases = [(dict(out=None), ARG, "out is NULL"),
             (dict(natoms=None), ARG, "natoms is NULL"),
             (dict(count=0), ARG, "num_graphs must be >= 1"),
             (dict(count=-1), ARG, "num_graphs must be >= 1"),
             (dict(natoms=i32([1, 0])), ARG, "natoms[1] must be >= 1"),
             (dict(natoms=i32([-5, 2])), ARG, "natoms[0] must be >= 1")]
    if holder:
        cases.append((dict(natoms=i32([1, 257])), UNSUPPORTED,
                      f"natoms[1] = 257: {holder} holds at most 256 atoms per crystal"))
    else:
        cases.append((dict(natoms=i32([2 ** 31 - 1, 1])), UNSUPPORTED, f"more than 2^31 - 1 atoms in one {plan}"))
    refused(lib, f"chm_{leg}_create", base, cases)
    assert h.value is None  # no plan came back


def test_match_create_refusals(lib):
    h = ctypes.c_void_p()
    base = dict(natoms=i32(NATOMS), count=B, ref_natoms=i32(REFS), refs=R, ref_of=i32(REF_OF), out=ctypes.byref(h))
    refused(lib, "chm_match_create", base, [
        (dict(out=None), ARG, "out is NULL"),
        (dict(natoms=None), ARG, "natoms is NULL"),
        (dict(ref_natoms=None), ARG, "ref_natoms is NULL"),
        (dict(ref_of=None), ARG, "ref_of is NULL"),
        (dict(count=0), ARG, "num_graphs must be >= 1"),
        (dict(refs=0), ARG, "num_refs must be >= 1"),
        (dict(natoms=i32([1, 0])), ARG, "natoms[1] must be >= 1"),
        (dict(ref_natoms=i32([0])), ARG, "ref_natoms[0] must be >= 1"),
        (dict(natoms=i32([1, 257])), UNSUPPORTED, "natoms[1] = 257: the matcher holds at most 256 atoms per crystal"),
        (dict(ref_natoms=i32([257])), UNSUPPORTED, "ref_natoms[0] = 257: the matcher holds at most 256 atoms per crystal"),
        (dict(ref_of=i32([-1, 1])), ARG, "ref_of[1] = 1 outside [-1, 1)"),
        (dict(ref_of=i32([-2, 0])), ARG, "ref_of[0] = -2 outside [-1, 1)"),
        # the first bad argument in the order of the checks is the one reported
        (dict(natoms=None, ref_natoms=None, count=0), ARG, "natoms is NULL"),
        (dict(ref_natoms=None, count=0), ARG, "ref_natoms is NULL"),
        (dict(natoms=i32([1, 0]), ref_natoms=i32([257])), ARG, "natoms[1] must be >= 1")])
    assert h.value is None


# ---------------------------------------------------------------- the entry points that launch
def state_cases(unit, first=()):
    """The refusals of the state's three buffers, shared by every leg that reads a state."""
    return list(first) + [
        (dict(a=None), ARG, "atom_types [N] is NULL"),
        (dict(n_a=4), ARG, f"atom_types [N]: 4 elements, {unit} needs 3"),
        (dict(x=None), ARG, "frac [N,3] is NULL"),
        (dict(n_x=8), ARG, f"frac [N,3]: 8 elements, {unit} needs 9"),
        (dict(lat=None), ARG, "lattices [B,3,3] is NULL"),
        (dict(n_lat=9), ARG, f"lattices [B,3,3]: 9 elements, {unit} needs 18")]


def tolerance_cases(name, top, tail):
    text = f"{name} must be in (0, {top:g}]{tail}"
    return [({name: v}, ARG, text) for v in (0.0, -0.1, top * 1.01, NAN, INF)]


def test_screen_run_refusals(lib, slots):
    plan = screen_module.screen_plan(NATOMS, DEV)
    base = dict(p=plan.handle, a=slots(0), n_a=N, x=slots(1), n_x=3 * N, lat=slots(2), n_lat=9 * B, target=None,
                n_target=0, max_length=60.0, min_distance=0.5, out=slots(3), n_out=64 * B, stream=_lib.stream_handle())
    refused(lib, "chm_screen_run", base, [(dict(p=None), ARG, "screen plan is NULL")] + state_cases("the screen") + [
        (dict(n_target=104), ARG, "target is NULL but 104 elements"),
        (dict(target=slots(4), n_target=5), ARG,
         "target: 5 elements, the screen needs 104 (one for all) or 208 ([B,104])"),
        (dict(max_length=0.0), ARG, "max_length must be > 0"),
        (dict(max_length=NAN), ARG, "max_length must be > 0"),
        (dict(min_distance=-1.0), ARG, "min_distance must be > 0"),
        (dict(min_distance=NAN), ARG, "min_distance must be > 0"),
        (dict(out=None), ARG, "out is NULL"),
        (dict(n_out=64), ARG, "out: 64 bytes, the screen needs 128"),
        (dict(out=slots(3, 4)), ARG, "out must be 16-byte aligned"),
        (dict(n_a=4, n_out=64, max_length=0.0), ARG, "atom_types [N]: 4 elements, the screen needs 3")])


def test_cell_refusals(lib, slots):
    plan = cell_module.cell_plan(NATOMS, DEV)
    unit = "the cell plan"
    base = dict(p=plan.handle, lat=slots(0), n_lat=9 * B, require=None, n_require=0, symprec=0.1, angle_tolerance=10.0,
                out=slots(1), n_out=128 * B, stream=_lib.stream_handle())
    refused(lib, "chm_cell_run", base, [
        (dict(p=None), ARG, "cell plan is NULL"),
        (dict(lat=None), ARG, "lattices [B,3,3] is NULL"),
        (dict(n_lat=9), ARG, f"lattices [B,3,3]: 9 elements, {unit} needs 18"),
        (dict(n_require=1), ARG, "require is NULL but 1 elements"),
        (dict(require=slots(2), n_require=3), ARG, f"require: 3 elements, {unit} needs 1 (one for all) or 2 ([B])"),
        (dict(require=slots(2), n_require=0), ARG, f"require: 0 elements, {unit} needs 1 (one for all) or 2 ([B])")] +
        tolerance_cases("symprec", 1.0, " A") + tolerance_cases("angle_tolerance", 30.0, " degrees") + [
        (dict(out=None), ARG, "out is NULL"),
        (dict(n_out=128), ARG, f"out: 128 bytes, {unit} needs 256"),
        (dict(out=slots(1, 4)), ARG, "out must be 16-byte aligned"),
        (dict(symprec=NAN, n_lat=9), ARG, f"lattices [B,3,3]: 9 elements, {unit} needs 18")])
    base = dict(p=plan.handle, rec=slots(0), n_rec=128 * B, x=slots(2), n_x=3 * N, lat=slots(3), n_lat=9 * B,
                x_out=slots(4), n_x_out=3 * N, lat_out=slots(5), n_lat_out=9 * B, stream=_lib.stream_handle())
    refused(lib, "chm_cell_apply", base, [
        (dict(p=None), ARG, "cell plan is NULL"),
        (dict(rec=None), ARG, "records is NULL"),
        (dict(n_rec=128), ARG, f"records: 128 bytes, {unit} needs 256"),
        (dict(rec=slots(0, 4)), ARG, "records must be 16-byte aligned"),
        (dict(x=None), ARG, "frac [N,3] is NULL"),
        (dict(n_x=8), ARG, f"frac [N,3]: 8 elements, {unit} needs 9"),
        (dict(lat=None), ARG, "lattices [B,3,3] is NULL"),
        (dict(n_lat=9), ARG, f"lattices [B,3,3]: 9 elements, {unit} needs 18"),
        (dict(x_out=None), ARG, "frac_out [N,3] is NULL"),
        (dict(n_x_out=8), ARG, f"frac_out [N,3]: 8 elements, {unit} needs 9"),
        (dict(lat_out=None), ARG, "lattices_out [B,3,3] is NULL"),
        (dict(n_lat_out=9), ARG, f"lattices_out [B,3,3]: 9 elements, {unit} needs 18"),
        (dict(x_out=slots(2)), ARG, "frac_out must not be frac: the cell is never applied in place"),
        (dict(lat_out=slots(3)), ARG, "lattices_out must not be lattices: the cell is never applied in place")])


def test_symm_run_refusals(lib, slots):
    plan = symmetry_module.symmetry_plan(NATOMS, DEV)
    unit = "the symmetry plan"
    base = dict(p=plan.handle, rec=slots(0), n_rec=128 * B, a=slots(2), n_a=N, x=slots(3), n_x=3 * N, lat=slots(4),
                n_lat=9 * B, require=None, n_require=0, symprec=0.1, angle_tolerance=10.0, out=slots(5), n_out=64 * B,
                ops=None, n_ops=0, stream=_lib.stream_handle())
    refused(lib, "chm_symm_run", base, [
        (dict(p=None), ARG, "symmetry plan is NULL"),
        (dict(rec=None), ARG, "cell records is NULL"),
        (dict(n_rec=128), ARG, f"cell records: 128 bytes, {unit} needs 256"),
        (dict(rec=slots(0, 4)), ARG, "cell records must be 16-byte aligned")] + state_cases(unit) + [
        (dict(n_require=2), ARG, "require is NULL but 2 elements"),
        (dict(require=slots(6), n_require=3), ARG, f"require: 3 elements, {unit} needs 1 (one for all) or 2 ([B])")] +
        tolerance_cases("symprec", 1.0, " A") + tolerance_cases("angle_tolerance", 30.0, " degrees") + [
        (dict(out=None), ARG, "out is NULL"),
        (dict(n_out=64), ARG, f"out: 64 bytes, {unit} needs 128"),
        (dict(out=slots(5, 4)), ARG, "out must be 16-byte aligned"),
        (dict(n_ops=16), ARG, "ops is NULL but 16 bytes"),
        (dict(ops=slots(8), n_ops=16), ARG, f"ops: 16 bytes, {unit} needs 1536"),
        (dict(ops=slots(8, 4), n_ops=1536), ARG, "ops must be 16-byte aligned")])


def test_dedup_refusals(lib, slots):
    plan = dedup_module.dedup_plan(NATOMS, DEV)
    unit, K = "the dedup", 8
    bins = [(dict(K=7), ARG, "K (bins per channel) must be in [8, 256], got 7"),
            (dict(K=257), ARG, "K (bins per channel) must be in [8, 256], got 257")]

    def positive(name):
        return [({name: v}, ARG, f"{name} must be positive and finite") for v in (0.0, -1.0, NAN, INF)]

    base = dict(p=plan.handle, a=slots(0), n_a=N, x=slots(1), n_x=3 * N, lat=slots(2), n_lat=9 * B, K=K, r_cut=6.0,
                sigma=0.15, fp=slots(3), n_fp=2 * K * B, counts=slots(4), n_counts=104 * B, flags=slots(8), n_flags=B,
                stream=_lib.stream_handle())
    refused(lib, "chm_dedup_fingerprint", base, bins + positive("r_cut") + positive("sigma") + state_cases(
        unit, [(dict(p=None), ARG, "dedup plan is NULL")]) + [
        (dict(fp=None), ARG, "fp [B,2K] is NULL"),
        (dict(n_fp=31), ARG, f"fp [B,2K]: 31 elements, {unit} needs 32"),
        (dict(counts=None), ARG, "counts [B,104] is NULL"),
        (dict(n_counts=104), ARG, f"counts [B,104]: 104 elements, {unit} needs 208"),
        (dict(flags=None), ARG, "flags [B] is NULL"),
        (dict(n_flags=3), ARG, f"flags [B]: 3 elements, {unit} needs 2"),
        (dict(p=None, K=7), ARG, "K (bins per channel) must be in [8, 256], got 7")])
    need = lib.chm_dedup_workspace_bytes(B)
    assert need > 0 and lib.chm_dedup_workspace_bytes(0) == 0
    base = dict(B=B, K=K, fp=slots(3), n_fp=2 * K * B, counts=slots(4), n_counts=104 * B, flags=slots(8), n_flags=B,
                exclude=None, n_exclude=0, tol=0.05, group=slots(9), n_group=B, count=slots(10), n_count=B,
                ws=slots(11), ws_bytes=need, stream=_lib.stream_handle())
    refused(lib, "chm_dedup_group", base, [
        (dict(B=0), ARG, "B must be >= 1"),
        (dict(B=65536 * 32), UNSUPPORTED, "more than 65535 * 32 fingerprints in one grouping")] + bins + positive("tol") + [
        (dict(fp=None), ARG, "fp [B,2K] is NULL"),
        (dict(n_fp=33), ARG, f"fp [B,2K]: 33 elements, {unit} needs 32"),
        (dict(counts=None), ARG, "counts [B,104] is NULL"),
        (dict(n_counts=0), ARG, f"counts [B,104]: 0 elements, {unit} needs 208"),
        (dict(flags=None), ARG, "flags is NULL but 2 elements"),
        (dict(n_flags=1), ARG, f"flags [B]: 1 elements, {unit} needs 2"),
        (dict(n_exclude=2), ARG, "exclude is NULL but 2 elements"),
        (dict(exclude=slots(12), n_exclude=3), ARG, f"exclude [B]: 3 elements, {unit} needs 2"),
        (dict(group=None), ARG, "group [B] is NULL"),
        (dict(n_group=1), ARG, f"group [B]: 1 elements, {unit} needs 2"),
        (dict(count=None), ARG, "count [B] is NULL"),
        (dict(n_count=3), ARG, f"count [B]: 3 elements, {unit} needs 2"),
        (dict(ws=None), ARG, "workspace is NULL"),
        (dict(ws_bytes=need - 1), ARG, f"workspace: {need - 1} bytes, {unit} needs {need}"),
        (dict(ws=slots(11, 2)), ARG, "workspace must be 4-byte aligned")])


def matcher_tolerances():
    return tolerance_cases("ltol", 1.0, "") + tolerance_cases("stol", 1.0, "") + \
        tolerance_cases("angle_tol", 30.0, " degrees")


def test_match_run_refusals(lib, slots):
    plan = match_module.match_plan(NATOMS, REFS, REF_OF, DEV)
    unit = "the match plan"
    base = dict(p=plan.handle, rec=slots(0), n_rec=128 * B, a=slots(2), n_a=N, x=slots(3), n_x=3 * N, lat=slots(4),
                n_lat=9 * B, rrec=slots(5), n_rrec=128 * R, ra=slots(6), n_ra=NR, rx=slots(7), n_rx=3 * NR,
                rlat=slots(8), n_rlat=9 * R, ltol=0.2, stol=0.3, angle_tol=5.0, out=slots(9), n_out=64 * B, perm=None,
                n_perm=0, stream=_lib.stream_handle())
    refused(lib, "chm_match_run", base, [
        (dict(p=None), ARG, "match plan is NULL"),
        (dict(rec=None), ARG, "cell records is NULL"),
        (dict(n_rec=128), ARG, f"cell records: 128 bytes, {unit} needs 256"),
        (dict(rec=slots(0, 4)), ARG, "cell records must be 16-byte aligned")] + state_cases(unit) + [
        (dict(rrec=None), ARG, "ref cell records is NULL"),
        (dict(n_rrec=64), ARG, f"ref cell records: 64 bytes, {unit} needs 128"),
        (dict(rrec=slots(5, 4)), ARG, "ref cell records must be 16-byte aligned"),
        (dict(ra=None), ARG, "ref_atom_types [NR] is NULL"),
        (dict(n_ra=3), ARG, f"ref_atom_types [NR]: 3 elements, {unit} needs 2"),
        (dict(rx=None), ARG, "ref_frac [NR,3] is NULL"),
        (dict(n_rx=9), ARG, f"ref_frac [NR,3]: 9 elements, {unit} needs 6"),
        (dict(rlat=None), ARG, "ref_lattices [R,3,3] is NULL"),
        (dict(n_rlat=18), ARG, f"ref_lattices [R,3,3]: 18 elements, {unit} needs 9")] + matcher_tolerances() + [
        (dict(out=None), ARG, "out is NULL"),
        (dict(n_out=64), ARG, f"out: 64 bytes, {unit} needs 128"),
        (dict(out=slots(9, 4)), ARG, "out must be 16-byte aligned"),
        (dict(n_perm=3), ARG, "perm is NULL but 3 elements"),
        (dict(perm=slots(10), n_perm=2), ARG, f"perm [N]: 2 elements, {unit} needs 3")])


def test_match_group_run_refusals(lib, slots):
    plan = match_group_module.match_group_plan(NATOMS, DEV)
    assert plan.num_pairs == 0
    unit, need = "the match plan", plan.workspace_bytes
    assert need == lib.chm_match_group_workspace_bytes(plan.handle) and need > 0
    assert lib.chm_match_group_workspace_bytes(None) == 0 and lib.chm_match_group_num_pairs(None) == 0
    base = dict(p=plan.handle, rec=slots(0), n_rec=128 * B, a=slots(2), n_a=N, x=slots(3), n_x=3 * N, lat=slots(4),
                n_lat=9 * B, exclude=None, n_exclude=0, ltol=0.2, stol=0.3, angle_tol=5.0, group=slots(5), n_group=B,
                count=slots(6), n_count=B, out=slots(7), n_out=32 * B, pairs=None, n_pairs=0, ws=slots(8),
                ws_bytes=need, stream=_lib.stream_handle())
    refused(lib, "chm_match_group_run", base, [
        (dict(p=None), ARG, "match-group plan is NULL"),
        (dict(rec=None), ARG, "cell records is NULL"),
        (dict(n_rec=128), ARG, f"cell records: 128 bytes, {unit} needs 256"),
        (dict(rec=slots(0, 4)), ARG, "cell records must be 16-byte aligned")] + state_cases(unit) + [
        (dict(n_exclude=2), ARG, "exclude is NULL but 2 elements"),
        (dict(exclude=slots(9), n_exclude=3), ARG, f"exclude [B]: 3 elements, {unit} needs 2")] +
        matcher_tolerances() + [
        (dict(group=None), ARG, "group [B] is NULL"),
        (dict(n_group=3), ARG, f"group [B]: 3 elements, {unit} needs 2"),
        (dict(count=None), ARG, "count [B] is NULL"),
        (dict(n_count=1), ARG, f"count [B]: 1 elements, {unit} needs 2"),
        (dict(out=None), ARG, "out is NULL"),
        (dict(n_out=32), ARG, f"out: 32 bytes, {unit} needs 64"),
        (dict(out=slots(7, 4)), ARG, "out must be 16-byte aligned"),
        (dict(n_pairs=16), ARG, "pair records: 16 bytes, the plan has no pair"),
        (dict(pairs=slots(10, 4)), ARG, "pair records must be 16-byte aligned"),
        (dict(ws=None), ARG, "workspace is NULL"),
        (dict(ws_bytes=need - 1), ARG, f"workspace: {need - 1} bytes, the match grouping needs {need}"),
        (dict(ws=slots(8, 4)), ARG, "workspace must be 16-byte aligned")])
    # a plan with one pair, for the pair records' own count
    paired = match_group_module.match_group_plan([2, 2], DEV)
    assert paired.num_pairs == 1
    base.update(p=paired.handle, n_a=4, n_x=12, pairs=slots(10), n_pairs=16, ws_bytes=paired.workspace_bytes)
    refused(lib, "chm_match_group_run", base, [
        (dict(pairs=None), ARG, "pair records is NULL"),
        (dict(n_pairs=8), ARG, f"pair records: 8 bytes, {unit} needs 16"),
        (dict(n_pairs=0), ARG, f"pair records: 0 bytes, {unit} needs 16"),
        (dict(pairs=slots(10, 4)), ARG, "pair records must be 16-byte aligned")])


# ---------------------------------------------------------------- the Python layer
def reference():
    return match_module.Reference(REFS, np.array([8, 8]), np.zeros((NR, 3), np.float32), np.eye(3, dtype=np.float32)[None])


def states():
    """name -> (call(natoms, a, x, lat), the dtype refusal, the leg reads atom_types)"""
    full = "the state must be atom_types int64, frac_coords / lattices float32"
    match = match_module.Match(reference(), ref_of=REF_OF)
    return {
        "screen": (lambda n, a, x, l: screen_module.screen_states(n, a, x, l), full, True),
        "cell": (lambda n, a, x, l: cell_module.cell_states(n, a, x, l), "the state must be frac_coords / lattices float32",
                 False),
        "symmetry": (lambda n, a, x, l: symmetry_module.symmetry_states(n, a, x, l), full, True),
        "dedup": (lambda n, a, x, l: dedup_module.fingerprint_states(n, a, x, l), full, True),
        "match": (lambda n, a, x, l: match_module.match_states(n, a, x, l, match), full, True),
        "match_group": (lambda n, a, x, l: match_group_module.match_group_states(n, a, x, l), full, True)}


def good_state(device=DEV):
    return (torch.zeros(N, dtype=torch.int64, device=device), torch.zeros(N, 3, device=device),
            torch.zeros(B, 3, 3, device=device))


LEGS = ["screen", "cell", "symmetry", "dedup", "match", "match_group"]
CPU_TEXT = "chemeleon_amd runs on a HIP device only: got a CPU tensor (no CPU fallback)"


def raises(kind, text, call, *args):
    with pytest.raises(kind) as e:
        call(*args)
    assert type(e.value) is kind and str(e.value) == text, (type(e.value), str(e.value))


@pytest.mark.parametrize("leg", LEGS)
def test_states_refuse_bad_states(leg):
    call, dtype_text, reads_types = states()[leg]
    a, x, lat = good_state()
    empty = "natoms must list at least one crystal of at least one atom"
    raises(ValueError, empty, call, [], a, x, lat)
    raises(ValueError, empty, call, [3, 0], a, x, lat)
    if leg in ("match", "match_group"):
        raises(ValueError, "the matcher holds at most 256 atoms per crystal, got 257", call, [1, 257], a, x, lat)
    shapes = "state shapes do not match natoms"
    raises(ValueError, shapes, call, NATOMS, a[:2], x, lat)
    raises(ValueError, shapes, call, NATOMS, a, x[:, :2], lat)
    raises(ValueError, shapes, call, NATOMS, a, x, lat[:1])
    raises(ValueError, shapes, call, [1, 1], a, x, lat)
    raises(ValueError, dtype_text, call, NATOMS, a, x.double(), lat)
    raises(ValueError, dtype_text, call, NATOMS, a, x, lat.half())
    if reads_types:
        raises(ValueError, dtype_text, call, NATOMS, a.int(), x, lat)
    ca, cx, cl = good_state("cpu")
    raises(RuntimeError, CPU_TEXT, call, NATOMS, a, cx, lat)
    raises(RuntimeError, CPU_TEXT, call, NATOMS, a, x, cl)
    raises(RuntimeError, CPU_TEXT, call, NATOMS, ca, x, lat)
    raises(RuntimeError, "chemeleon_amd expects contiguous tensors", call, NATOMS, a, x.t().contiguous().t(), lat)


@pytest.mark.parametrize("leg", LEGS)
def test_states_refuse_mixed_devices(leg):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    call, _, reads_types = states()[leg]
    a, x, lat = good_state("cuda:0")
    text = "the state's tensors are on different devices"
    raises(ValueError, text, call, NATOMS, a, x, lat.to("cuda:1"))
    if reads_types:
        raises(ValueError, text, call, NATOMS, a.to("cuda:1"), x, lat)


def test_exclude_is_validated_before_anything_runs():
    a, x, lat = good_state()
    group = match_group_module.match_group_states
    raises(ValueError, "exclude has shape (3,), the state lists 2 crystals", group, NATOMS, a, x, lat, None,
           np.zeros(3, dtype=bool))
    raises(ValueError, "exclude has shape (2, 1), the state lists 2 crystals", group, NATOMS, a, x, lat, None,
           torch.zeros(2, 1, dtype=torch.bool))
    raises(ValueError, "exclude must be bool or uint8", group, NATOMS, a, x, lat, None, np.zeros(2, dtype=np.float32))
    fps = dedup_module.Fingerprints(torch.zeros(B, 128, device=DEV), torch.zeros(B, 104, dtype=torch.int32, device=DEV),
                                    torch.zeros(B, dtype=torch.int32, device=DEV))
    fingerprints = dedup_module.group_fingerprints
    raises(ValueError, "exclude has shape (3,), the fingerprints list 2 crystals", fingerprints, fps, None, [0, 1, 0])
    raises(ValueError, "exclude must be bool or uint8", fingerprints, fps, None, torch.zeros(2, dtype=torch.int64))


# ---------------------------------------------------------------- the plan caches
PLAN_FUNCTIONS = {"screen": screen_module.screen_plan, "cell": cell_module.cell_plan,
                  "symmetry": symmetry_module.symmetry_plan, "dedup": dedup_module.dedup_plan,
                  "match": lambda natoms, device: match_module.match_plan(natoms, REFS, [0] * len(natoms), device),
                  "match_group": match_group_module.match_group_plan}


@pytest.mark.parametrize("leg", LEGS)
def test_plan_cache_keeps_the_last_eight(leg):
    def plan(natoms):
        return PLAN_FUNCTIONS[leg](natoms, DEV)

    first = plan([5, 9])  # (lists no other test uses: every key below is new to the cache)
    assert plan([5, 9]) is first and plan((5, 9)) is first
    others = [plan([5, 9, k]) for k in range(1, 8)]
    assert plan([5, 9]) is first  # seven newer keys: still held
    assert all(plan([5, 9, k]) is others[k - 1] for k in range(1, 8))
    plan([5, 9, 8])  # the eighth pushes the oldest out
    again = plan([5, 9])  # a new plan, which in turn pushes out [5, 9, 1] and nothing else
    assert again is not first and again.natoms == first.natoms == (5, 9)
    assert plan([5, 9, 2]) is others[1]
    assert plan([5, 9, 1]) is not others[0]
    raises(RuntimeError, "chemeleon_amd runs on a HIP device only: got cpu", PLAN_FUNCTIONS[leg], [1], "cpu")
