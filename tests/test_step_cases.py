"""The CPU side of the update-kernel tests (tests/step_cases.py, tests/test_gpu_step_update.py): the float32
restatement is OracleModel.step bit for bit, the guidance weights of the ABI and of the reference differ exactly
where the issue says, every planted edge is hit, every node of every case counts under the gap rule, and
chm_debug_step_update refuses bad arguments before any HIP call (so those checks run here without a device)."""

import ctypes
import functools

import pytest
import torch

from chemeleon_amd import _lib
from oracle import chemeleon_oracle as O
from tests import step_cases as S

A, T = S.A, S.T


@functools.lru_cache(maxsize=None)
def _ref():
    ref = S.oracle_model()
    return ref, S.coef_table(ref)


def _noise(d, t):
    return (d["ra"], d["rl"], d["rx1"], d["rx2"]) if t > 1 else None


def _oracle_step(ref, nat, t, d, cond_scale, patch):
    """OracleModel.step on prepared decoder outputs. patch = "model_predictions": the method returns the mixed
    tensors (the restatement's mix with the reference's weights); patch = "decoder": the decoder returns the raw
    outputs, cond then null, so that the oracle's own mix runs too."""
    B, N = len(nat), sum(nat)
    n2g = torch.arange(B).repeat_interleave(torch.tensor(nat))
    w = S.weights(cond_scale, abi=False)
    calls = []
    if patch == "model_predictions":
        def fake(self, te, a, x, l, natoms, n2g_, cs, cond, null):
            calls.append(1)
            if len(calls) == 1:
                return S.mix(d["types"], w), S.mix(d["lattice"], w), S.mix(d["coords"], w)
            return None, None, S.mix(d["coords2"], w)
    else:
        def fake(self, te, a, x, l, natoms, n2g_, text):
            calls.append(1)
            k = (len(calls) - 1) % 2  # cond, null, cond, null
            if len(calls) <= 2:
                return d["types"][k], d["lattice"][k], d["coords"][k], None
            return torch.zeros(N, A), torch.zeros(B, 3, 3), d["coords2"][k], None
    saved = getattr(O.OracleModel, patch)
    setattr(O.OracleModel, patch, fake)
    try:
        out = ref.step(t, d["a"], d["x"], d["l"], torch.tensor(nat), n2g, None, None, _noise(d, t), cond_scale,
                       S.STEP_LR)
    finally:
        setattr(O.OracleModel, patch, saved)
    assert len(calls) == (2 if patch == "model_predictions" else 4)
    return out


def _restated_step(ref, coef, nat, t, d, w):
    N = sum(nat)
    nz = _noise(d, t) or (None,) * 4
    a_prev = S.types32(torch.full((N,), t), d["a"], d["types"], nz[0], ref.q_one_step, ref.q_mats, w)
    x_half, l_prev = S.predictor(t, d["x"], d["l"], d["coords"], d["lattice"], nz[1], nz[2], coef, w)
    x_prev = S.corrector(t, x_half, d["coords2"], nz[3], coef, w)
    return a_prev, x_prev, l_prev, x_half


@pytest.mark.parametrize("patch", ["model_predictions", "decoder"])
@pytest.mark.parametrize("t", S.TS)
@pytest.mark.parametrize("name", ["1", "ragged", "1x29"])
def test_restatement_is_the_oracle_step(name, t, patch):
    ref, coef = _ref()
    nat = S.SHAPES[name]
    d = S.inputs(nat, t, S.seed_of(name, t), coef)
    want = _oracle_step(ref, nat, t, d, 2.0, patch)
    got = _restated_step(ref, coef, nat, t, d, S.weights(2.0))
    assert torch.equal(got[0], want[0]), "atom types"
    for g, w_, what in zip(got[1:], want[1:], ("x_prev", "l_prev", "x_half")):
        assert g.dtype == torch.float32 and torch.equal(S.bits(g), S.bits(w_)), f"{what} differs from OracleModel.step"


def test_null_weight_deviation_at_cond_scale_1_3():
    """The ABI takes cond_scale as a float and forms the null weight from it; the reference forms 1 - cond_scale
    in double from the Python float. Equal at 2.0, 1.0, 0.0; at 1.3 they are -0.29999995 and -0.30000001. The
    oracle at 1.3 is the restatement with the reference's weights, bit for bit, and not with the ABI's."""
    for cs in (2.0, 1.0, 0.0):
        assert S.weights(cs, abi=True) == S.weights(cs, abi=False)
    w_abi, w_ref = S.weights(1.3, abi=True), S.weights(1.3, abi=False)
    print(f"cond_scale 1.3: null weight ABI {w_abi[0]!r} reference {w_ref[0]!r}; cond weight {w_abi[1]!r}")
    assert w_abi[1] == w_ref[1]
    assert w_abi[0] != w_ref[0]
    assert f"{w_abi[0]:.8f}" == "-0.29999995" and f"{w_ref[0]:.8f}" == "-0.30000001"
    ref, coef = _ref()
    nat, t = S.SHAPES["ragged"], 50
    d = S.inputs(nat, t, S.seed_of("ragged", t), coef, w_abi)
    want = _oracle_step(ref, nat, t, d, 1.3, "decoder")
    got = _restated_step(ref, coef, nat, t, d, w_ref)
    for g, w_ in zip(got[1:], want[1:]):
        assert torch.equal(S.bits(g), S.bits(w_))
    # (at t = 50 the coefficients swallow the difference; it shows in the mix itself)
    assert not torch.equal(S.mix(d["types"], w_abi), S.mix(d["types"], w_ref)), "the two weights give the same mix"


MASKED = [(0, 1), (2, 0), (2, 1)]


@pytest.mark.parametrize("name,nat,t", [pytest.param(n, nat, t, id=f"{n}-t{t}") for n, nat, t in S.cases()])
def test_every_edge_is_hit(name, nat, t):
    """From the reference alone: what the GPU tests rely on is in the inputs."""
    ref, coef = _ref()
    w = S.weights(2.0)
    d = S.inputs(nat, t, S.seed_of(name, t), coef, w)
    N = sum(nat)
    pl = S.mix(d["lattice"], w)
    for i, j in MASKED:  # non-zero l, pl and noise at the masked lattice positions
        assert bool((d["l"][:, i, j] != 0).all()) and bool((pl[:, i, j] != 0).all()) and bool((d["rl"][:, i, j] != 0).all())
    if t >= T - 1:  # the clip engages at both ends at T; the same inputs at T - 1 leave [-6, 6] unclipped
        dT = S.inputs(nat, T, S.seed_of(name, T), coef, w)
        for k in d:
            if k != "wrap_edges":
                assert torch.equal(S.bits(d[k]) if d[k].is_floating_point() else d[k],
                                   S.bits(dT[k]) if d[k].is_floating_point() else dT[k]), k
        raw = S.predictor(T, d["x"], d["l"], d["coords"], d["lattice"], d["rl"], d["rx1"], coef, w, clip=False)[1]
        cut = S.predictor(T, d["x"], d["l"], d["coords"], d["lattice"], d["rl"], d["rx1"], coef, w)[1]
        assert float(raw.max()) > 6 and float(raw.min()) < -6
        assert float(cut.max()) == 6 and float(cut.min()) == -6
        assert 0 < abs(float(cut[0, 2, 2])) < 6 and float(cut[0, 2, 2]) == float(raw[0, 2, 2])
        prev = S.predictor(T - 1, d["x"], d["l"], d["coords"], d["lattice"], d["rl"], d["rx1"], coef, w)[1]
        assert float(prev.max()) > 6 and float(prev.min()) < -6
    # the corrector's wrap edges: the unwrapped value is the planted one, bit for bit
    edges = d["wrap_edges"]
    assert len(edges) == min(3 * N, len(S.WRAP_EDGES))
    raw = S.corrector(t, d["x2"], d["coords2"], d["rx2"] if t > 1 else None, coef, w, wrap=False).view(-1)
    if t > 1:  # (at t == 1 the noise is not read: -0.0 + 0.0 is then +0.0, still the 0 edge)
        assert torch.equal(S.bits(raw[:len(edges)]), S.bits(torch.tensor(edges)))
    else:
        assert torch.equal(raw[:len(edges)], torch.tensor(edges))
    wrapped = (raw % 1.0)[:len(edges)]
    for v, r in zip(edges, wrapped.tolist()):
        if v == -1.0e-9:
            assert r == 1.0  # torch's % 1.0 returns exactly 1.0 for a tiny negative
        elif v in (0.0, 1.0):
            assert r == 0.0
    assert int(d["a"][0]) in (0, A - 1) if N == 1 else (int(d["a"].min()) == 0 and int(d["a"].max()) == A - 1)
    if t == 1:
        cls, *_ = S.type_decisions(torch.full((N,), t), d["a"], d["types"], None, ref.q_one_step, ref.q_mats, w)
        assert int(cls[N // 2]) == S.NAN_CLASS


def test_wrap_edges_all_occur():
    """The one-atom batch holds three of the six edges and one of x_t = 0 / A - 1 per case; over its cases all occur."""
    _ref_, coef = _ref()
    seen, xt = set(), set()
    for t in S.TS:
        d = S.inputs([1], t, S.seed_of("1", t), coef)
        seen |= {repr(v) for v in d["wrap_edges"]}
        xt.add(int(d["a"][0]))
    assert seen == {repr(v) for v in S.WRAP_EDGES} and xt == {0, A - 1}


def _all_count(t_node, a, types, ra, q1, qm, w, what):
    cls, ok, gap, thr = S.type_decisions(t_node, a, types, ra, q1, qm, w)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} nodes are near ties (gap {gap[~ok].tolist()}, bound {thr[~ok].tolist()})"


@pytest.mark.parametrize("name,nat,t", [pytest.param(n, nat, t, id=f"{n}-t{t}") for n, nat, t in S.cases()])
def test_every_node_counts(name, nat, t):
    """No node of any case is a near tie of the float64 scores, so the GPU tests compare every node."""
    ref, coef = _ref()
    N = sum(nat)
    tn = torch.full((N,), t)
    scales = S.COND_SCALES if (name == "ragged" and t in S.SCALE_TS) else (2.0,)
    for cs in scales:
        w = S.weights(cs)
        d = S.inputs(nat, t, S.seed_of(name, t), coef, w)
        _all_count(tn, d["a"], d["types"], d["ra"] if t > 1 else None, ref.q_one_step, ref.q_mats, w,
                   f"{name} t {t} scale {cs}")
        if t == 1:  # (the device-t run reads finite noise at t == 1 and multiplies it by 0: the same decisions)
            _all_count(tn, d["a"], d["types"], d["ra"], ref.q_one_step, ref.q_mats, w, f"{name} t 1 with noise")


@pytest.mark.parametrize("A_", S.D3PM_A)
def test_every_d3pm_node_counts(A_):
    ref, _coef = _ref()
    q1, qm = S.d3pm_tables(ref, A_)
    for N in S.D3PM_N:
        lg, xt, tn, u = S.d3pm_inputs(A_, N, S.d3pm_seed(A_, N))
        assert int(xt[0]) == 0 and (N == 1 or int(xt[-1]) == A_ - 1)
        if N >= 4:
            assert {1, 2, T} <= set(tn.tolist())
        _all_count(tn, xt, lg, u, q1, qm, None, f"A {A_} N {N}")
        if A_ > 1:  # the float32 oracle decides as float64 does
            cls, *_ = S.type_decisions(tn, xt, lg, u, q1, qm, None)
            assert torch.equal(cls, O.d3pm_p_sample(lg, xt, tn, u, q1, qm))


# ---------------------------------------------------------------- chm_debug_step_update refuses bad arguments (no device)
def _call(b=None, sched="ok", t=50, d_t=None, io="ok", stage=1, types=0x40000, coords=0x50000, lattice=0x60000,
          noise=0, T_=T, tables=True):
    lib = _lib.load()
    x = 0x10000  # (never dereferenced: every refusal comes before the first HIP call)
    sc = _lib.chm_schedule(T_, A, 128, 0, x if tables else None, x, x, x) if sched == "ok" else None
    st = _lib.chm_step_io()
    st.d_atom_types, st.d_frac, st.d_lattices = x, x, x
    for k, name in enumerate(("d_rand_a", "d_rand_l", "d_rand_x1", "d_rand_x2")):
        if noise & (1 << k):
            setattr(st, name, x)
    rc = lib.chm_debug_step_update(b, ctypes.byref(sc) if sc is not None else None, t, d_t, 2.0,
                                   ctypes.byref(st) if io == "ok" else None, 0, 0, 0, types, 6 * A, coords, 18, lattice,
                                   18, stage, None)
    return rc, lib.chm_last_error()


@pytest.mark.parametrize("kw,field", [
    (dict(sched=None), b"schedule"), (dict(io=None), b"io"), (dict(stage=0), b"stage"), (dict(stage=3), b"stage"),
    (dict(t=0), b"t 0 outside"), (dict(t=T + 1), b"outside"), (dict(T_=0), b"T must be"),
    (dict(tables=False), b"schedule table"), (dict(noise=1), b"all four"), (dict(noise=7), b"all four"),
    (dict(coords=None), b"d_coords"), (dict(coords=None, stage=2), b"d_coords"), (dict(types=None), b"d_types"),
    (dict(lattice=None), b"d_lattice"), (dict(), b"batch"), (dict(t=0, d_t=0x70000), b"batch"),
    (dict(stage=2, types=None, lattice=None), b"batch"), (dict(noise=15), b"batch"),
])
def test_debug_step_update_refuses_bad_arguments_without_a_device(kw, field):
    rc, err = _call(**kw)
    assert rc == -1, (kw, err)  # CHM_E_ARG, not a HIP error: no HIP call was made
    assert b"chm_debug_step_update" in err and field in err, (kw, err)
