"""The CPU side of the training-kernel tests (tests/train_cases.py, tests/test_gpu_train_kernels.py): the float32
restatement is d3pm_q_sample and OracleModel.training_forward bit for bit, every planted edge is hit, every node of
every case counts under the gap rule (the planted exact ties aside), and chm_debug_train_update refuses bad
arguments before any HIP call (so those checks run here without a device)."""

import ctypes

import pytest
import torch

from chemeleon_amd import _lib
from oracle import chemeleon_oracle as O
from tests import train_cases as C

CASES = [pytest.param(n, T, A, id=f"{n}-T{T}-A{A}") for n, _nat, T, A in C.cases()]


def _oracle_forward(ref, d):
    """OracleModel.training_forward with a decoder that returns d's outputs and records the noised state."""
    seen = {}

    def fake(self, te, a, x, l, natoms, n2g, text):
        seen.update(a_t=a, x_t=x, l_t=l)
        return d["types"], d["lattice"], d["coords"], None

    saved = O.OracleModel.decoder
    O.OracleModel.decoder = fake
    try:
        out = ref.training_forward(d["a0"], d["x0"], d["l0"], d["nat"], d["t"], d["ra"], d["nl"], d["nx"], None)
    finally:
        O.OracleModel.decoder = saved
    return out, seen


@pytest.mark.parametrize("name,T,A", CASES)
def test_restatement_is_the_oracle(name, T, A):
    ref = C.ref_model(T, A)
    for k in C.ROTATIONS[name]:
        d = C.inputs(name, T, A, k)
        want, seen = _oracle_forward(ref, d)
        tn = d["t"][d["n2g"]]
        a_t = torch.argmax(C.q_scores(ref, d), dim=-1)
        assert torch.equal(a_t, O.d3pm_q_sample(d["a0"], tn, d["ra"], ref.q_mats)), "q_sample"
        assert torch.equal(a_t, want["x_t_atom_types"]) and torch.equal(a_t, seen["a_t"])
        assert torch.equal(a_t, C.a_t_decisions(ref, d)[0]), "the float32 q_sample decides as float64 does"
        r = C.reference(ref, d, torch.float32)
        for key, w in (("x_t", seen["x_t"]), ("l_t", seen["l_t"]), ("target", want["true_noise_coords"]),
                       ("loss", want["loss"]), ("vb_loss", want["vb_loss_atom_types"]),
                       ("ce_loss", want["ce_loss_atom_types"])):
            assert r[key].dtype == torch.float32 and torch.equal(C.bits(r[key]), C.bits(w)), f"k {k}: {key}"
        # (loss pins its three parts; the per-node values are the terms of the two means)
        assert torch.equal(C.bits(r["kl"].mean()), C.bits(want["vb_loss_atom_types"]))
        assert abs(float(r["ce"].double().mean()) - float(want["ce_loss_atom_types"])) <= 1e-6 * float(r["ce"].abs().max())


def _hits(ref, d):
    """The planted edges a case holds, found from the reference's results alone."""
    a0, ra, ty = d["a0"], d["ra"], d["types"]
    a_t, _ok, tie = C.a_t_decisions(ref, d)
    r64 = C.noised(ref, d, torch.float64)
    hit = set()
    pl = d["plants"]

    def at(p):
        return pl.get(p, -1)

    if at("a0_absorbed") >= 0 and int(a0[at("a0_absorbed")]) == 0:
        hit.add("a0_absorbed")
    j = at("xt_is_a0")
    if j >= 0 and int(a_t[j]) == int(a0[j]) != 0 and bool((ra[j] == 1.0).any()):
        hit.add("xt_is_a0")
    j = at("xt_absorbed")
    if j >= 0 and int(a_t[j]) == 0 != int(a0[j]):
        hit.add("xt_absorbed")
    j = at("xt_neither")
    if j >= 0 and int(a_t[j]) not in (0, int(a0[j])):
        hit.add("xt_neither")
    j = at("two_ones")
    if j >= 0 and int((ra[j] == 1.0).sum()) == 2 and bool(tie[j]) and int(a_t[j]) == 1:
        hit.add("two_ones")
    j = at("uniform_zero")
    if j >= 0 and bool((ra[j] == 0.0).any()):
        hit.add("uniform_zero")
    j = at("logits_80")
    if j >= 0 and float(ty[j].max()) == 80.0 and float(ty[j].min()) == -80.0:
        hit.add("logits_80")
    j = at("constant_row")
    if j >= 0 and bool((ty[j] == ty[j, 0]).all()):
        hit.add("constant_row")
    j = at("p_a0_underflows")
    if j >= 0 and float(torch.softmax(ty[j], -1)[a0[j]]) == 0.0 and float(torch.softmax(ty[j].double(), -1)[a0[j]]) > 0.0:
        hit.add("p_a0_underflows")
    assert int(tie.sum()) == (1 if "two_ones" in pl else 0), "an exact tie that was not planted"
    # node 0's coordinates: wraps from below, the largest float below 1, wraps from above
    s = ref.sigmas[d["t"][0]].double()
    raw = d["x0"][0].double() + s * d["nx"][0].double()
    assert float(d["x0"][0, 0]) == 0.0 and float(raw[0]) < 0.0 and 0.0 < float(r64["x_t"][0, 0]) < 1.0
    assert float(d["x0"][0, 1]) == C.X0_TOP < 1.0
    assert float(raw[2]) >= 1.0
    return hit, set(d["t"].tolist()), r64["rs"]


def test_every_edge_is_hit():
    """From the reference alone: what the GPU tests rely on is in the inputs. A batch of nine nodes or more holds
    every plant in each of its cases, the one-atom batch one per case and all of them over its cases; every shape
    runs every timestep over its rotations; both branches of the score target's comparison occur."""
    one_hits = set()
    for _n, _nat, T, A in C.cases():
        if _n != "1":
            continue
        ref = C.ref_model(T, A)
        for name in C.SHAPES:
            ts = set()
            for k in C.ROTATIONS[name]:
                hit, tk, rs = _hits(ref, C.inputs(name, T, A, k))
                ts |= tk
                if name == "1":
                    assert len(hit) == 1
                    one_hits |= hit
                else:
                    assert hit == set(C.PLANTS), (name, T, A, k, set(C.PLANTS) - hit)
                    assert bool((rs >= 1e-2).any()) and bool((rs < 1e-2).any())
            assert ts == set(C.timesteps(T)), (name, T, A, ts)
    assert one_hits == set(C.PLANTS), set(C.PLANTS) - one_hits


def test_shapes_are_what_the_kernels_need():
    N, B = sum(C.BIG), len(C.BIG)
    assert B >= 33 and N >= 258 and N % 4 and 9 * B > 256 and min(C.BIG) == 1 and max(C.BIG) == 12
    assert sum(C.SHAPES["ragged"]) % 4 and 1 in C.SHAPES["ragged"]


@pytest.mark.parametrize("name,T,A", CASES)
def test_every_node_counts(name, T, A):
    """No node of any case is a near tie of the float64 q_sample scores, so the GPU tests compare every node."""
    ref = C.ref_model(T, A)
    for k in C.ROTATIONS[name]:
        _cls, ok, _tie = C.a_t_decisions(ref, C.inputs(name, T, A, k))
        assert bool(ok.all()), f"{name} T {T} A {A} k {k}: nodes {torch.nonzero(~ok).view(-1).tolist()} are near ties"


# ---------------------------------------------------------------- chm_debug_train_update refuses bad arguments (no device)
ARGS = ("d_t", "d_a0", "d_x0", "d_l0", "d_rand_a", "d_noise_l", "d_noise_x", "d_types", "d_coords", "d_lattice",
        "d_out", "d_a_t", "d_x_t", "d_l_t", "d_target_x", "d_part")


def _call(tables="ok", T_=100, table_ptr=True, **null):
    lib = _lib.load()
    x = 0x10000  # (never dereferenced: every refusal comes before the first HIP call)
    tt = _lib.chm_train_tables(T_, x if table_ptr else None, x, x, 1.0, 1.0, 1.0, 1.0) if tables == "ok" else None
    p = {k: (None if null.get(k) else x) for k in ARGS}
    rc = lib.chm_debug_train_update(None, ctypes.byref(tt) if tt is not None else None, p["d_t"], p["d_a0"], p["d_x0"],
                                    p["d_l0"], p["d_rand_a"], p["d_noise_l"], p["d_noise_x"], p["d_types"], 104,
                                    p["d_coords"], 3, p["d_lattice"], 9, p["d_out"], p["d_a_t"], p["d_x_t"],
                                    p["d_l_t"], p["d_target_x"], p["d_part"], None)
    return rc, lib.chm_last_error()


@pytest.mark.parametrize("kw,field", [
    (dict(tables=None), b"tables"), (dict(T_=0), b"T must be"), (dict(table_ptr=False), b"NULL table"),
    (dict(d_t=1), b"d_t"), (dict(d_a0=1), b"d_a0"), (dict(d_x0=1), b"d_x0"), (dict(d_l0=1), b"d_l0"),
    (dict(d_rand_a=1), b"all three"), (dict(d_noise_l=1), b"all three"), (dict(d_noise_x=1), b"all three"),
    (dict(d_types=1), b"d_types"), (dict(d_coords=1), b"d_coords"), (dict(d_lattice=1), b"d_lattice"),
    (dict(d_out=1), b"d_out"), (dict(d_a_t=1), b"noised-state"), (dict(d_x_t=1), b"noised-state"),
    (dict(d_l_t=1), b"noised-state"), (dict(d_target_x=1), b"noised-state"), (dict(d_part=1), b"d_part"),
    (dict(), b"batch"),
])
def test_debug_train_update_refuses_bad_arguments_without_a_device(kw, field):
    rc, err = _call(**kw)
    assert rc == -1, (kw, err)  # CHM_E_ARG, not a HIP error: no HIP call was made
    assert b"chm_debug_train_update" in err and field in err, (kw, err)
