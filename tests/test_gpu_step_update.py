"""The reverse step's update kernels (k_step_predictor, k_d3pm as the step calls it, k_step_corrector;
csrc/kernels.hip) through chm_debug_step_update, which runs them with sample_step's own arguments on caller-supplied
decoder outputs, against the CPU reference of tests/step_cases.py (pinned to the oracle by tests/test_step_cases.py).

Coordinates and lattices equal the float32 restatement BIT FOR BIT (bit patterns: a signed zero at a masked lattice
entry counts). Atom types are compared as decisions with the float64 scores, on every node: the seeds are chosen so
that no node is a near tie (test_step_cases.py::test_every_node_counts). Each comparison prints its largest ulp
distance before it asserts (pytest -s); the table is in profiles/r11/step_unit/README.md.

Guards: sentinel rows behind every state buffer must stay untouched. A HIP error from the hook ends the session:
nothing else runs on the device after a fault. Run on an MI355X: pytest -m gpu."""

import ctypes
import functools

import pytest
import torch

from chemeleon_amd import _lib

from . import step_cases as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
A, T = S.A, S.T
SENTINEL_ROWS = 8
SENT_A, SENT_F = -7777, -123.25
CASES = [pytest.param(n, nat, t, id=f"{n}-t{t}") for n, nat, t in S.cases()]


@pytest.fixture(scope="module")
def model():
    """As tests/test_abi.py::_gpu_batch: synthetic weights, timesteps = 100; split16, the default math."""
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict
    cfg = default_config()
    cfg["timesteps"] = T
    torch.manual_seed(0)
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    m = m.to(DEV).eval()
    assert m.decoder.get_math() == "split16"
    return m


@pytest.fixture(scope="module")
def ref():
    return S.oracle_model()


@pytest.fixture(scope="module")
def coef(model, ref):
    """The reference's coefficient table; the device reads the model's, which must be the same bit for bit."""
    c = S.coef_table(ref)
    _sched, (coef_d, _temb, q1, qm) = model.schedule_tables(S.STEP_LR)
    assert torch.equal(S.bits(coef_d.cpu()), S.bits(c))
    assert torch.equal(q1.cpu(), ref.q_one_step) and torch.equal(qm.cpu(), ref.q_mats)
    return c


@pytest.fixture(scope="module")
def batches(model):
    cache = {}

    def get(nat, pairs=2):
        key = (tuple(nat), pairs)
        if key not in cache:
            cache[key] = model.decoder.hip_batch(list(nat), max_pairs=pairs, private=True)
        return cache[key]

    return get


@functools.lru_cache(maxsize=None)
def _inputs_cached(name, t, cs):
    ref = S.oracle_model()
    nat = S.BIG if name == "big" else S.SHAPES[name]
    return S.inputs(nat, t, S.seed_of(name, t), S.coef_table(ref), S.weights(cs))


def padded(t, rows, fill):
    """A device copy of t with SENTINEL_ROWS rows of `fill` behind it."""
    out = torch.full((t.shape[0] + rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    out[:t.shape[0]] = t.to(DEV)
    return out


def update(model, b, t, cs, state, outs, stage, noise=None, d_t=None, seed=0, node_base=0, graph_base=0):
    """One chm_debug_step_update call on device copies of state = (a, x, l) with sentinel rows behind them; outs =
    (types, coords, lattice) CPU tensors (None allowed at stage 2). Returns the new (a, x, l) on the CPU."""
    lib = _lib.load()
    a, x, l = state
    N, B = a.shape[0], l.shape[0]
    ab, xb, lb = padded(a, SENTINEL_ROWS, SENT_A), padded(x.float(), SENTINEL_ROWS, SENT_F), padded(l.float(), SENTINEL_ROWS, SENT_F)
    nz = None if noise is None else [z.to(DEV).float().contiguous() for z in noise]
    io = _lib.step_io(ab, xb, lb, noise=nz, nodes=N, graphs=B)
    o = [None if v is None else v.to(DEV).float().contiguous() for v in outs]
    sched, _keep = model.schedule_tables(S.STEP_LR)
    n = [0 if v is None else v.numel() for v in o]
    rc = lib.chm_debug_step_update(b.handle, sched, t, _lib.ptr(d_t), cs, ctypes.byref(io), seed, node_base, graph_base,
                                   _lib.ptr(o[0]), n[0], _lib.ptr(o[1]), n[1], _lib.ptr(o[2]), n[2], stage,
                                   _lib.stream_handle())
    if rc == -2:  # CHM_E_HIP: nothing else runs on the device after a fault
        pytest.exit(f"chm_debug_step_update: {lib.chm_last_error().decode(errors='replace')}", returncode=3)
    assert rc == 0, lib.chm_last_error()
    ab, xb, lb = ab.cpu(), xb.cpu(), lb.cpu()
    assert bool((ab[N:] == SENT_A).all()) and bool((xb[N:] == SENT_F).all()) and bool((lb[B:] == SENT_F).all()), \
        "rows behind the state were written"
    return ab[:N], xb[:N], lb[:B]


def same_bits(got, want, what, check=True):
    """Bit equality, after printing how far apart the two are. check=False: print and return the verdict."""
    eq = torch.equal(S.bits(got), S.bits(want))
    if eq:
        print(f"{what}: bit-identical")
    else:
        fin = torch.isfinite(got) & torch.isfinite(want)
        u = S.ulps(got[fin], want[fin])
        print(f"{what}: {int((S.bits(got) != S.bits(want)).sum())} of {got.numel()} elements differ, max "
              f"{int(u.max()) if u.numel() else -1} ulp, non-finite mismatches {int((~fin).sum())}")
    assert eq or not check, f"{what} differs from the float32 restatement"
    return eq


def decisions(ref, d, t, w, N, noise=True):
    cls, ok, _gap, _thr = S.type_decisions(torch.full((N,), t), d["a"], d["types"], d["ra"] if noise else None,
                                           ref.q_one_step, ref.q_mats, w)
    assert bool(ok.all())  # (test_step_cases.py::test_every_node_counts)
    return cls


def nan_noise(d):
    return [torch.full_like(d[k], float("nan")) for k in ("ra", "rl", "rx1", "rx2")]


def run_predictor(model, b, ref, coef, d, t, cs, w, **kw):
    """Stage 1 with explicit noise at host t (at t == 1: NaN-filled buffers, which must not be read). Returns the
    device's (a, x, l) and the reference's (classes, x_half, l_prev)."""
    N = d["a"].shape[0]
    noise = nan_noise(d) if t == 1 else [d["ra"], d["rl"], d["rx1"], d["rx2"]]
    got = update(model, b, t, cs, (d["a"], d["x"], d["l"]), (d["types"], d["coords"], d["lattice"]), 1, noise, **kw)
    rl, rx1 = (None, None) if t == 1 else (d["rl"], d["rx1"])
    x_half, l_prev = S.predictor(t, d["x"], d["l"], d["coords"], d["lattice"], rl, rx1, coef, w)
    return got, (decisions(ref, d, t, w, N, noise=t > 1), x_half, l_prev)


# ------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("name,nat,t", CASES)
def test_predictor_bit_for_bit(model, batches, ref, coef, name, nat, t):
    """k_step_predictor's coordinates and lattices equal the restatement bit for bit, the clip at t == T and the
    masked entries' signed zeros included; k_d3pm's classes are the float64 decisions on every node."""
    d = _inputs_cached(name, t, 2.0)
    w = S.weights(2.0)
    (a, x, l), (cls, x_half, l_prev) = run_predictor(model, batches(nat), ref, coef, d, t, 2.0, w)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(l).all())
    assert torch.equal(a, cls), f"{name} t {t}: {int((a != cls).sum())} of {a.numel()} atom types differ"
    ok_l = same_bits(l, l_prev, f"{name} t {t} lattices", check=False)
    same_bits(x, x_half, f"{name} t {t} coordinates")
    assert ok_l, f"{name} t {t} lattices differ from the float32 restatement"


@pytest.mark.parametrize("name,nat,t", CASES)
def test_corrector_bit_for_bit(model, batches, ref, coef, name, nat, t):
    """k_step_corrector: the Langevin move and the wrap, the planted wrap edges among its inputs."""
    d = _inputs_cached(name, t, 2.0)
    w = S.weights(2.0)
    noise = nan_noise(d) if t == 1 else [d["ra"], d["rl"], d["rx1"], d["rx2"]]
    state = (d["a"], d["x2"], d["l"])
    a, x, l = update(model, batches(nat), t, 2.0, state, (None, d["coords2"], None), 2, noise)
    assert torch.equal(a, d["a"]) and torch.equal(S.bits(l), S.bits(d["l"])), "stage 2 wrote types or lattices"
    same_bits(x, S.corrector(t, d["x2"], d["coords2"], None if t == 1 else d["rx2"], coef, w), f"{name} t {t} wrapped coordinates")


# ------------------------------------------------------------------------------------------ cond_scale
def _err(got, want64, periodic=False):
    e = (got.double() - want64).abs()
    if periodic:
        e = torch.minimum(e, 1.0 - e)
    return float(e.max())


@pytest.mark.parametrize("cs", S.COND_SCALES)
@pytest.mark.parametrize("t", S.SCALE_TS)
def test_cond_scale(model, batches, ref, coef, t, cs):
    """Both stages against the restatement with the ABI's weights, bit for bit. At 1.3 the ABI's null weight is not
    the reference's (test_step_cases.py): there the result is also held against the float64 chain with the
    reference's weights, within 16 x the error of the float32 restatement with the reference's weights against that
    same chain, per output tensor (the margin the edge-layer tests give a float32 baseline)."""
    nat = S.SHAPES["ragged"]
    d = _inputs_cached("ragged", t, cs)
    w = S.weights(cs)
    b = batches(nat)
    (a, x, l), (cls, x_half, l_prev) = run_predictor(model, b, ref, coef, d, t, cs, w)
    assert torch.equal(a, cls)
    ok_l = same_bits(l, l_prev, f"scale {cs} t {t} lattices", check=False)
    ok_x = same_bits(x, x_half, f"scale {cs} t {t} coordinates", check=False)
    noise = nan_noise(d) if t == 1 else [d["ra"], d["rl"], d["rx1"], d["rx2"]]
    _a, x2, _l = update(model, b, t, cs, (d["a"], d["x2"], d["l"]), (None, d["coords2"], None), 2, noise)
    rx2 = None if t == 1 else d["rx2"]
    ok_c = same_bits(x2, S.corrector(t, d["x2"], d["coords2"], rx2, coef, w), f"scale {cs} t {t} wrapped coordinates",
                     check=False)
    assert ok_l and ok_x and ok_c, f"scale {cs} t {t}: lattices {ok_l}, coordinates {ok_x}, wrapped coordinates {ok_c}"
    if cs != 1.3:
        return
    wr = S.weights(cs, abi=False)
    rl, rx1 = (None, None) if t == 1 else (d["rl"], d["rx1"])
    f64, f32 = torch.float64, torch.float32
    xh64, l64 = S.predictor(t, d["x"], d["l"], d["coords"], d["lattice"], rl, rx1, coef, wr, f64)
    xh32, l32 = S.predictor(t, d["x"], d["l"], d["coords"], d["lattice"], rl, rx1, coef, wr, f32)
    xc64 = S.corrector(t, d["x2"], d["coords2"], rx2, coef, wr, f64)
    xc32 = S.corrector(t, d["x2"], d["coords2"], rx2, coef, wr, f32)
    for what, got, r32, r64, per in (("lattices", l, l32, l64, False), ("coordinates", x, xh32, xh64, False),
                                     ("wrapped coordinates", x2, xc32, xc64, True)):
        e, base = _err(got, r64, per), _err(r32, r64, per)
        print(f"scale 1.3 t {t} {what}: device error {e:.3e}, float32 baseline {base:.3e}, ratio "
              f"{e / base if base > 0 else float('inf') if e > 0 else 0.0:.2f}")
        assert e <= 16 * base, f"{what}: {e:.3e} against 16 x {base:.3e}"


# ------------------------------------------------------------------------------------------ chm_d3pm_sample
@pytest.mark.parametrize("A_", S.D3PM_A)
def test_d3pm_sample_direct(ref, A_):
    """The model-free entry point at the edges of the two-classes-per-lane layout, per-node t in {1, 2, T, ...}."""
    lib = _lib.load()
    q1, qm = S.d3pm_tables(ref, A_)
    q1d, qmd = q1.to(DEV).contiguous(), qm.to(DEV).contiguous()
    for N in S.D3PM_N:
        lg, xt, tn, u = S.d3pm_inputs(A_, N, S.d3pm_seed(A_, N))
        cls, ok, _gap, _thr = S.type_decisions(tn, xt, lg, u, q1, qm, None)
        assert bool(ok.all())
        out = torch.full((N + SENTINEL_ROWS,), SENT_A, dtype=torch.long, device=DEV)
        dv = [v.to(DEV).contiguous() for v in (lg, xt, tn, u)]
        rc = lib.chm_d3pm_sample(N, A_, T, _lib.ptr(dv[0]), _lib.ptr(dv[1]), _lib.ptr(dv[2]), _lib.ptr(dv[3]),
                                 _lib.ptr(q1d), _lib.ptr(qmd), _lib.ptr(out), _lib.stream_handle())
        if rc == -2:
            pytest.exit(f"chm_d3pm_sample: {lib.chm_last_error().decode(errors='replace')}", returncode=3)
        assert rc == 0, lib.chm_last_error()
        out = out.cpu()
        assert bool((out[N:] == SENT_A).all())
        assert torch.equal(out[:N], cls), f"A {A_} N {N}: {out[:N].tolist()} against {cls.tolist()}"


# ------------------------------------------------------------------------------------------ device t, Philox
@pytest.mark.parametrize("t", (100, 2, 1))
def test_device_t(model, batches, ref, coef, t):
    """t read from device memory gives what the host t gives, bit for bit, and is not decremented. At t == 1 the
    buffers hold finite noise, as the header requires (the atom-type uniforms are read and multiplied by 0)."""
    nat = S.SHAPES["ragged"]
    d = _inputs_cached("ragged", t, 2.0)
    w = S.weights(2.0)
    b = batches(nat)
    d_t = torch.full((1,), t, dtype=torch.int32, device=DEV)
    (a0, x0, l0), (cls, x_half, l_prev) = run_predictor(model, b, ref, coef, d, t, 2.0, w)
    a1, x1, l1 = update(model, b, 0, 2.0, (d["a"], d["x"], d["l"]), (d["types"], d["coords"], d["lattice"]), 1,
                        [d["ra"], d["rl"], d["rx1"], d["rx2"]], d_t=d_t)
    assert torch.equal(a1, a0) and torch.equal(a1, cls)
    assert torch.equal(S.bits(x1), S.bits(x0)) and torch.equal(S.bits(l1), S.bits(l0))
    noise = [d["ra"], d["rl"], d["rx1"], d["rx2"]]
    state = (d["a"], d["x2"], d["l"])
    _a, xh, _l = update(model, b, t, 2.0, state, (None, d["coords2"], None), 2, nan_noise(d) if t == 1 else noise)
    _a, xd, _l = update(model, b, 0, 2.0, state, (None, d["coords2"], None), 2, noise, d_t=d_t)
    assert torch.equal(S.bits(xd), S.bits(xh))
    assert int(d_t) == t


def philox(seed, t, kind, base, n, normal):
    out = torch.empty(n, device=DEV)
    _lib.check(_lib.load().chm_debug_philox(seed, t, kind, base, n, normal, _lib.ptr(out), _lib.stream_handle()),
               "chm_debug_philox")
    return out.cpu()


@pytest.mark.parametrize("t", (50, 2))
def test_philox_noise(model, batches, t):
    """Without noise buffers the kernels draw streams 0-3 at (node_base + i) * 128 + class, (graph_base + g) * 9 + q
    and (node_base + i) * 3 + k (twice): the result equals the explicit-noise run fed from chm_debug_philox, with
    bases that need the 64-bit index arithmetic."""
    nat = S.SHAPES["ragged"]
    N, B = sum(nat), len(nat)
    d = _inputs_cached("ragged", t, 2.0)
    b = batches(nat)
    seed, node_base, graph_base = 77, 2 ** 33 + 5, 2 ** 31 + 3
    ra = philox(seed, t, 0, node_base * 128, N * 128, 0).view(N, 128)[:, :A].contiguous()
    assert torch.equal(ra.view(-1), torch.from_numpy(S.philox_uniform(
        seed, t, 0, (torch.arange(N)[:, None] + node_base).numpy().astype("uint64") * 128 + torch.arange(A).numpy().astype("uint64"))).view(-1))
    rl = philox(seed, t, 1, graph_base * 9, B * 9, 1).view(B, 3, 3)
    rx1 = philox(seed, t, 2, node_base * 3, N * 3, 1).view(N, 3)
    rx2 = philox(seed, t, 3, node_base * 3, N * 3, 1).view(N, 3)
    s1, o1 = (d["a"], d["x"], d["l"]), (d["types"], d["coords"], d["lattice"])
    s2, o2 = (d["a"], d["x2"], d["l"]), (None, d["coords2"], None)
    kw = dict(seed=seed, node_base=node_base, graph_base=graph_base)
    for state, outs, stage in ((s1, o1, 1), (s2, o2, 2)):
        want = update(model, b, t, 2.0, state, outs, stage, [ra, rl, rx1, rx2])
        got = update(model, b, t, 2.0, state, outs, stage, None, **kw)
        assert torch.equal(got[0], want[0]), f"stage {stage} atom types"
        assert torch.equal(S.bits(got[1]), S.bits(want[1])), f"stage {stage} coordinates"
        assert torch.equal(S.bits(got[2]), S.bits(want[2])), f"stage {stage} lattices"
        other = update(model, b, t, 2.0, state, outs, stage, None, seed=seed, node_base=node_base + 1, graph_base=graph_base)
        assert not torch.equal(S.bits(other[1]), S.bits(want[1])), "another base is another stream"


# ------------------------------------------------------------------------------------------ the hook is the step
@pytest.mark.parametrize("t", (50, 1))
def test_hook_is_the_step(model, batches, t):
    """chm_sample_step against chm_decoder_forward (pairs = 2), hook stage 1, chm_decoder_forward, hook stage 2:
    all three state tensors bit-identical (the corrector's reuse of the FiLM conditioning included)."""
    from chemeleon_amd.synthetic import synthetic_text_embeds
    lib = _lib.load()
    nat = S.SHAPES["ragged"]
    N, B = sum(nat), len(nat)
    d = _inputs_cached("ragged", t, 2.0)
    b = batches(nat)
    sched, (_coef, temb, _q1, _qm) = model.schedule_tables(S.STEP_LR)
    cond, null = (v.to(DEV).float().expand(B, -1).contiguous() for v in synthetic_text_embeds(512))
    a0, x0, l0 = d["a"], d["x"], (d["l"] * S.O.LATTICE_MASK).contiguous()
    noise = None if t == 1 else [d[k].to(DEV).contiguous() for k in ("ra", "rl", "rx1", "rx2")]
    st = _lib.stream_handle()
    # the step
    a, x, l = a0.to(DEV).clone(), x0.to(DEV).clone(), l0.to(DEV).clone()
    _lib.check(lib.chm_sample_step(b.handle, sched, t, 2.0, ctypes.byref(_lib.step_io(a, x, l, cond, null, noise)),
                                   0, 0, 0, st), "chm_sample_step")
    torch.cuda.synchronize()
    want = (a.cpu(), x.cpu(), l.cpu())
    # its pieces
    text = torch.stack([cond, null], 0).contiguous()
    te = _lib.ptr(temb, t * temb.shape[1] * 4)

    def forward(a_, x_, l_):
        ty = torch.empty(2, N, A, device=DEV)
        la = torch.empty(2, B, 3, 3, device=DEV)
        co = torch.empty(2, N, 3, device=DEV)
        _lib.check(lib.chm_decoder_forward(b.handle, 2, _lib.ptr(a_), _lib.ptr(x_), _lib.ptr(l_), te, 0, _lib.ptr(text),
                                           _lib.ptr(ty), _lib.ptr(la), _lib.ptr(co), None, st), "chm_decoder_forward")
        torch.cuda.synchronize()
        return ty.cpu(), co.cpu(), la.cpu()

    nz = None if t == 1 else [d[k] for k in ("ra", "rl", "rx1", "rx2")]
    s1 = update(model, b, t, 2.0, (a0, x0, l0), forward(a0.to(DEV), x0.to(DEV), l0.to(DEV)), 1, nz)
    o2 = forward(*(v.to(DEV).contiguous() for v in s1))
    got = update(model, b, t, 2.0, s1, (None, o2[1], None), 2, nz)
    assert torch.equal(got[0], want[0]), "atom types"
    assert torch.equal(S.bits(got[2]), S.bits(want[2])), "lattices"
    assert torch.equal(S.bits(got[1]), S.bits(want[1])), "coordinates"


# ------------------------------------------------------------------------------------------ refusals on a real batch
def test_hook_refuses_what_the_batch_cannot_take(model, batches):
    lib = _lib.load()
    nat = S.SHAPES["ragged"]
    N, B = sum(nat), len(nat)
    a = torch.zeros(N, dtype=torch.long, device=DEV)
    x = torch.zeros(N, 3, device=DEV)
    l = torch.zeros(B, 3, 3, device=DEV)
    ty, co, la = torch.zeros(2, N, A, device=DEV), torch.zeros(2, N, 3, device=DEV), torch.zeros(2, B, 3, 3, device=DEV)
    sched, _keep = model.schedule_tables(S.STEP_LR)

    def call(b=None, sc=sched, n_types=ty.numel(), n_coords=co.numel(), n_lattice=la.numel(), io=None):
        io = _lib.step_io(a, x, l) if io is None else io
        return lib.chm_debug_step_update((b or batches(nat)).handle, sc, 50, None, 2.0, ctypes.byref(io), 0, 0, 0,
                                         _lib.ptr(ty), n_types, _lib.ptr(co), n_coords, _lib.ptr(la), n_lattice, 1,
                                         _lib.stream_handle())

    assert call(b=batches(nat, 1)) == -1 and b"max_pairs" in lib.chm_last_error()
    assert call(n_types=N * A) == -1 and b"n_types" in lib.chm_last_error()
    assert call(n_coords=3 * N) == -1 and b"n_coords" in lib.chm_last_error()
    assert call(n_lattice=9 * B) == -1 and b"n_lattice" in lib.chm_last_error()
    io = _lib.step_io(a, x, l)
    io.n_frac = 3 * N - 3
    assert call(io=io) == -1 and b"frac" in lib.chm_last_error()
    bad = _lib.chm_schedule(sched.T, 50, sched.time_dim, 0, sched.d_coef, sched.d_time_emb, sched.d_q_one_step,
                            sched.d_q_mats)
    assert call(sc=bad) == -1 and b"num_classes" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert bool((x == 0).all()) and bool((l == 0).all()) and bool((a == 0).all())  # (nothing ran)
    assert call() == 0, lib.chm_last_error()
