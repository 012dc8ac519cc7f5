"""Constrained sampling on the GPU (csrc/constrain.hip, chm_constrain_state, chm_sample_step_con,
Chemeleon.sample_states(constraint=...)) against the CPU reference of tests/constraint_cases.py.
Run on an MI355X: pytest -m gpu."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import Constraint, _lib

from . import constraint_cases as C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
A, T = C.A, C.T
SENTINEL_ROWS = 8


@pytest.fixture(scope="module")
def model():
    """As tests/test_abi.py::_gpu_batch: synthetic weights, timesteps = 100."""
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict
    cfg = default_config()
    cfg["timesteps"] = T
    torch.manual_seed(0)
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def ref():
    return C.oracle_model()


@pytest.fixture(scope="module")
def tables(ref):
    return C.tables_of(ref)


@pytest.fixture(scope="module")
def fwd_d(model, tables):
    """The model's own forward table on the device; it must be the reference's, bit for bit."""
    _tt, (coef, _q1, qm) = model._train_tables()
    assert torch.equal(coef.cpu(), tables["fwd"])
    assert torch.equal(qm.cpu(), tables["q_mats"])
    return coef


@pytest.fixture(scope="module")
def batches(model):
    cache = {}

    def get(nat, pairs=1):
        key = (tuple(nat), pairs)
        if key not in cache:
            cache[key] = model.decoder.hip_batch(list(nat), max_pairs=pairs, private=True)
        return cache[key]

    return get


def con_struct(con, fwd, noise=None):
    """chm_constraint with every pair given (also under an all-false mask: the kernel then reads the masks)."""
    bufs = [con.atom_types.to(DEV), con.type_mask.to(torch.uint8).to(DEV), con.frac_coords.to(DEV),
            con.frac_mask.to(torch.uint8).to(DEV), con.lattices.to(DEV), con.lattice_mask.to(torch.uint8).to(DEV)]
    c = _lib.chm_constraint()
    for name, t in zip(("a0", "type_mask", "x0", "frac_mask", "l0", "lattice_mask"), bufs):
        setattr(c, "d_" + name, t.data_ptr())
        setattr(c, "n_" + name, t.numel())
    c.d_fwd, c.n_fwd = fwd.data_ptr(), fwd.numel()
    if noise is not None:
        nz = [z.to(DEV).float().contiguous() for z in noise]
        for name, t in zip(("rand_a", "rand_l", "rand_x"), nz):
            setattr(c, "d_" + name, t.data_ptr())
            setattr(c, "n_" + name, t.numel())
        bufs += nz
    return c, bufs


SENT_A, SENT_F = -7777, -123.25


def padded_state(state):
    """Device copies of (a, x, l) with SENTINEL_ROWS rows of sentinels behind each, and the io over the real rows."""
    a, x, l = state
    N, B = a.shape[0], l.shape[0]
    ab = torch.full((N + SENTINEL_ROWS,), SENT_A, dtype=torch.long, device=DEV)
    xb = torch.full((N + SENTINEL_ROWS, 3), SENT_F, device=DEV)
    lb = torch.full((B + SENTINEL_ROWS, 3, 3), SENT_F, device=DEV)
    ab[:N], xb[:N], lb[:B] = a.to(DEV), x.to(DEV), l.to(DEV)
    return (ab, xb, lb), _lib.step_io(ab, xb, lb, nodes=N, graphs=B)


def check_padded(bufs, N, B, want, what=""):
    ab, xb, lb = (t.cpu() for t in bufs)
    assert bool((ab[N:] == SENT_A).all()) and bool((xb[N:] == SENT_F).all()) and bool((lb[B:] == SENT_F).all()), \
        f"{what}: rows behind the state were written"
    for got, ref_, name in zip((ab[:N], xb[:N], lb[:B]), want, ("types", "coordinates", "lattices")):
        assert torch.equal(got, ref_), f"{what}: {name} differ from the reference"


def constrain(model, b, c, level, what, io, seed=0, node_base=0, graph_base=0, d_t=None):
    sched, _keep = model.schedule_tables(1e-5)
    return _lib.load().chm_constrain_state(b.handle, sched, ctypes.byref(c), level, _lib.ptr(d_t), what,
                                           ctypes.byref(io), seed, node_base, graph_base, _lib.stream_handle())


# ------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("mask", C.KERNEL_MASKS)
@pytest.mark.parametrize("N", C.KERNEL_NODES)
def test_kernel_explicit_noise(model, batches, tables, fwd_d, N, mask):
    """Every field equals replace() bit for bit (unmasked entries therefore bit-unchanged); nothing behind the
    state is written."""
    for n_, mask_, level, seed in C.kernel_cases():
        if (n_, mask_) != (N, mask):
            continue
        nat, state, con, noise = C.kernel_inputs(N, mask, seed)
        b = batches(nat)
        c, _keep = con_struct(con, fwd_d, noise)
        bufs, io = padded_state(state)
        assert constrain(model, b, c, level, 7, io) == 0, _lib.load().chm_last_error()
        torch.cuda.synchronize()
        check_padded(bufs, N, len(nat), C.replace(level, state, con, noise, tables), f"N={N} {mask} level {level}")
    # the level read from device memory: s = *d_t - 1
    nat, state, con, noise = C.kernel_inputs(N, mask, C.KERNEL_SEED + 1000)
    if mask != "none":
        assert float(C.type_score_gaps(50, con, noise[0], tables).min()) >= 1e-3
    c, _keep = con_struct(con, fwd_d, noise)
    bufs, io = padded_state(state)
    d_t = torch.full((1,), 51, dtype=torch.int32, device=DEV)
    assert constrain(model, batches(nat), c, 0, 7, io, d_t=d_t) == 0, _lib.load().chm_last_error()
    torch.cuda.synchronize()
    check_padded(bufs, N, len(nat), C.replace(50, state, con, noise, tables), f"N={N} {mask} device t")
    assert int(d_t) == 51


def philox(seed, t, kind, base, n, normal):
    out = torch.empty(n, device=DEV)
    _lib.check(_lib.load().chm_debug_philox(seed, t, kind, base, n, normal, _lib.ptr(out), _lib.stream_handle()),
               "chm_debug_philox")
    return out.cpu()


@pytest.mark.parametrize("N,level,seed,node_base,graph_base", C.PHILOX_CASES)
def test_kernel_philox(model, batches, tables, fwd_d, N, level, seed, node_base, graph_base):
    """Without noise buffers the kernel draws streams 4 / 5 / 6 at (node_base + i) * 128 + class,
    (graph_base + g) * 9 + q, (node_base + i) * 3 + k with the step's t = level + 1 in the key."""
    nat, state, con, _noise = C.kernel_inputs(N, "all", seed)
    B, t = len(nat), level + 1
    u = philox(seed, t, 4, node_base * 128, N * 128, 0).view(N, 128)[:, :A].contiguous()
    assert torch.equal(u, C.philox_type_uniforms(seed, t, node_base, N)), "the host restatement of stream 4"
    zl = philox(seed, t, 5, graph_base * 9, B * 9, 1).view(B, 3, 3)
    zx = philox(seed, t, 6, node_base * 3, N * 3, 1).view(N, 3)
    b = batches(nat)
    c, _keep = con_struct(con, fwd_d)
    bufs, io = padded_state(state)
    assert constrain(model, b, c, level, 7, io, seed, node_base, graph_base) == 0, _lib.load().chm_last_error()
    torch.cuda.synchronize()
    want = C.replace(level, state, con, (u, zl, zx), tables)
    check_padded(bufs, N, B, want, f"philox N={N} level {level}")
    # what = 4: coordinates only, the same values
    bufs, io = padded_state(state)
    assert constrain(model, b, c, level, 4, io, seed, node_base, graph_base) == 0
    torch.cuda.synchronize()
    check_padded(bufs, N, B, (state[0], want[1], state[2]), f"philox what=4 N={N} level {level}")
    # another base is another stream
    bufs, io = padded_state(state)
    assert constrain(model, b, c, level, 4, io, seed, node_base + 1, graph_base) == 0
    torch.cuda.synchronize()
    if level > 0:
        assert not torch.equal(bufs[1][:N].cpu(), want[1])


def test_type_distribution(model, batches, tables, fwd_d):
    """65 536 nodes of known type 8 at the level where q_mats[s-1][8][8] is nearest 0.5: the Gumbel argmax samples
    in proportion to q + 1e-6, so class 8 has N p +- 5 binomial sigma nodes, and the classes outside {0, 8}
    together 102e-6 / (1 + 104e-6) of them (6.7 expected; at most 30)."""
    N = 1 << 16
    q = tables["q_mats"][:T, 8, 8]
    s = int(torch.argmin((q - 0.5).abs())) + 1
    p = float(tables["q_mats"][s - 1, 8, 8])
    nat = [1] * N
    con = Constraint.composition(nat, [[8]] * N)
    c, _keep = con_struct(con, fwd_d)
    a = torch.full((N,), 5, dtype=torch.long, device=DEV)
    x = torch.zeros(N, 3, device=DEV)
    l = torch.zeros(N, 3, 3, device=DEV)
    io = _lib.step_io(a, x, l)
    assert constrain(model, batches(nat), c, s, 1, io, seed=17) == 0, _lib.load().chm_last_error()
    counts = np.bincount(a.cpu().numpy(), minlength=A)
    other = int(counts.sum() - counts[0] - counts[8])
    print(f"level {s}: p {p:.4f}, class 8 {counts[8]} of {N} (expected {N * p:.0f} +- {np.sqrt(N * p * (1 - p)):.0f}), "
          f"outside {{0, 8}}: {other}")
    assert abs(counts[8] - N * p) <= 5 * np.sqrt(N * p * (1 - p))
    assert other <= 30
    assert bool((x == 0).all()) and bool((l == 0).all())


@pytest.mark.parametrize("kind", [5, 6])
def test_constraint_normal_streams(kind):
    """Streams 5 and 6 are standard normal, as tests/test_gpu_noise.py checks streams 1-3."""
    stats = pytest.importorskip("scipy.stats")
    n = 1 << 22
    z = philox(11, 321, kind, 0, n, 1).numpy().astype(np.float64)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2 / n)
    skew, kurt = stats.skew(z), stats.kurtosis(z)
    assert abs(skew) < 5 * np.sqrt(6 / n) and abs(kurt) < 5 * np.sqrt(24 / n)
    ks = stats.kstest(z, "norm")
    print(f"normal kind {kind}: mean {z.mean():.2e} var {z.var():.6f} KS D {ks.statistic:.2e} p {ks.pvalue:.3f}")
    assert ks.pvalue > 1e-3


# ------------------------------------------------------------------------------------------ the whole step
def scaled_err(gpu, ref_):
    gpu, ref_ = np.asarray(gpu, dtype=np.float64), np.asarray(ref_, dtype=np.float64)
    scale = max(np.sqrt(np.mean(ref_ ** 2)), 1e-12)
    return np.abs(gpu - ref_) / np.maximum(np.abs(ref_), scale)


@pytest.mark.parametrize("t", C.STEP_TS)
@pytest.mark.parametrize("nat", C.STEP_NATOMS, ids=lambda n: "x".join(map(str, n)))
def test_step_matches_reference(model, ref, tables, fwd_d, nat, t):
    """reverse_step with explicit step noise and constraint noise against constrained_step. Free entries: the
    teacher-forced step gates of tests/test_gpu_parity.py (types exact, coordinates 1e-4 periodic, lattices 1e-4);
    held entries bit for bit."""
    (a, x, l), nz, con, cnz = C.step_inputs(nat, t)
    B = len(nat)
    n = torch.tensor(nat)
    n2g = torch.arange(B).repeat_interleave(n)
    cond, null = C.conditioning(B)
    want = C.constrained_step(ref, t, a, x, l, n, n2g, cond, null, nz, con, cnz, tables)
    ga, gx, gl = (v.cpu() for v in model.reverse_step(t, a, x, l, nat, 2.0, 1e-5, cond[:1], null[:1], noise=nz,
                                                      constraint=con, constraint_noise=cnz))
    tm, fm, lm = con.type_mask, con.frac_mask, con.lattice_mask
    assert torch.equal(ga[tm], want[0][tm]) and torch.equal(gx[fm], want[1][fm]) and torch.equal(gl[lm], want[2][lm])
    assert torch.equal(ga[~tm], want[0][~tm]), "free atom types"
    d = (gx[~fm].double() - want[1][~fm].double()).abs()
    d = torch.minimum(d, 1 - d)
    dx = float(d.max()) if d.numel() else 0.0
    dl = float(scaled_err(gl[~lm], want[2][~lm]).max()) if bool((~lm).any()) else 0.0
    print(f"natoms {nat} t={t}: free coordinates {dx:.2e}, free lattices {dl:.2e}")
    assert dx <= C.STEP_GATE and dl <= C.STEP_GATE


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_field_and_touch_nothing(model, batches, fwd_d):
    lib = _lib.load()
    nat, state, con, noise = C.kernel_inputs(5, "all", 1)
    N, B = 5, len(nat)
    b = batches(nat)
    bufs, io = padded_state(state)
    before = [t.clone() for t in bufs]

    def refused(c, word, level=50, what=7, io_=io):
        assert constrain(model, b, c, level, what, io_) == -1, word
        assert word in lib.chm_last_error(), (word, lib.chm_last_error())

    for field, n_bad, word in [("n_a0", N - 1, b"a0"), ("n_type_mask", N + 1, b"type_mask"), ("n_x0", N, b"x0"),
                               ("n_frac_mask", 0, b"frac_mask"), ("n_l0", B, b"l0"),
                               ("n_lattice_mask", B + 1, b"lattice_mask"), ("n_rand_a", N * 100, b"rand_a"),
                               ("n_rand_l", 9 * B - 1, b"rand_l"), ("n_rand_x", N, b"rand_x"),
                               ("n_fwd", 4 * T, b"fwd"), ("n_fwd", 4 * (T + 2), b"fwd")]:
        c, _keep = con_struct(con, fwd_d, noise)
        setattr(c, field, n_bad)
        refused(c, word)
        assert b"elements" in lib.chm_last_error()
    for half in ("d_a0", "d_type_mask", "d_x0", "d_frac_mask", "d_l0", "d_lattice_mask"):
        c, _keep = con_struct(con, fwd_d, noise)
        setattr(c, half, None)
        refused(c, b"together")
    for drop in ("d_rand_a", "d_rand_l", "d_rand_x"):
        c, _keep = con_struct(con, fwd_d, noise)
        setattr(c, drop, None)
        refused(c, b"all three")
    c, _keep = con_struct(con, fwd_d, noise)
    refused(c, b"level", level=T + 1)
    refused(c, b"level", level=-1)
    refused(c, b"what", what=0)
    refused(c, b"what", what=8)
    short = _lib.step_io(bufs[0], bufs[1], bufs[2], nodes=N - 1, graphs=B)
    refused(c, b"atom_types", io_=short)
    sched, _k = model.schedule_tables(1e-5)
    st = _lib.stream_handle()
    assert lib.chm_constrain_state(b.handle, sched, None, 50, None, 7, ctypes.byref(io), 0, 0, 0, st) == -1
    assert b"constraint is NULL" in lib.chm_last_error()
    # the step entry point: the same checks, and con == NULL is refused
    b2 = batches(nat, 2)
    cond = torch.zeros(B, 512, device=DEV)
    sio = _lib.step_io(bufs[0], bufs[1], bufs[2], cond, cond, nodes=N, graphs=B)
    assert lib.chm_sample_step_con(b2.handle, sched, 50, None, 2.0, ctypes.byref(sio), None, 0, 0, 0, st) == -1
    assert b"constraint is NULL" in lib.chm_last_error()
    c, _keep = con_struct(con, fwd_d, noise)
    c.n_x0 = 3
    assert lib.chm_sample_step_con(b2.handle, sched, 50, None, 2.0, ctypes.byref(sio), ctypes.byref(c), 0, 0, 0,
                                   st) == -1
    assert b"x0" in lib.chm_last_error()
    torch.cuda.synchronize()
    for got, want in zip(bufs, before):
        assert torch.equal(got, want), "a refused call wrote to the state"


# ------------------------------------------------------------------------------------------ the loop
LOOP_NAT = [6, 6, 6, 6]


def loop_constraint():
    """Crystals 0 and 2: all types; the lattice of crystal 0; three coordinates (atoms) of crystal 2."""
    g = torch.Generator().manual_seed(77)
    N, B = 24, 4
    a0 = torch.randint(1, A, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g) * 2 - 0.5
    l0 = torch.randn(B, 3, 3, generator=g)
    tm, fm, lm = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)
    tm[0:6] = True
    tm[12:18] = True
    lm[0] = True
    fm[[12, 14, 17]] = True
    return Constraint(LOOP_NAT, a0, tm, x0, fm, l0, lm)


def held_ok(state, con):
    _t, a, x, l = state
    a, x, l = a.cpu(), x.cpu(), l.cpu()
    mask9 = model_mask()
    assert torch.equal(a[con.type_mask], con.atom_types[con.type_mask])
    assert torch.equal(l[con.lattice_mask], (con.lattices * mask9)[con.lattice_mask])
    assert torch.equal(x[con.frac_mask], (con.frac_coords % 1.0)[con.frac_mask])


def model_mask():
    from oracle import chemeleon_oracle as O
    return O.LATTICE_MASK


@pytest.fixture(scope="module")
def loop_runs(model):
    cond, null = C.conditioning(1)
    con = loop_constraint()
    kw = dict(noise="philox", seed=31, text_embeds=cond, null_text_embeds=null, clone=True)
    runs = {"eager": list(model.sample_states(LOOP_NAT, None, 2.0, 1e-5, graph=False, constraint=con, **kw)),
            "graph": list(model.sample_states(LOOP_NAT, None, 2.0, 1e-5, graph=True, constraint=con, **kw)),
            "free": list(model.sample_states(LOOP_NAT, None, 2.0, 1e-5, graph=True, **kw))}
    return con, runs


def test_loop_holds_the_known_entries(loop_runs):
    con, runs = loop_runs
    for name in ("eager", "graph"):
        assert runs[name][-1][0] == 0 and len(runs[name]) == T + 1
        held_ok(runs[name][-1], con)
    # and something was generated around them: the free run's crystals 0 and 2 differ
    assert not torch.equal(runs["graph"][-1][1][:6], runs["free"][-1][1][:6])


def test_loop_leaves_other_crystals_alone(loop_runs):
    """Crystals 1 and 3 carry no known entry: bit-identical at every step to the run without a constraint."""
    _con, runs = loop_runs
    for sc, sf in zip(runs["graph"], runs["free"]):
        assert sc[0] == sf[0]
        for rows in (slice(6, 12), slice(18, 24)):
            assert torch.equal(sc[1][rows], sf[1][rows]) and torch.equal(sc[2][rows], sf[2][rows]), f"t={sc[0]}"
        for g in (1, 3):
            assert torch.equal(sc[3][g], sf[3][g]), f"t={sc[0]} lattice {g}"


def test_loop_graph_replay_matches_eager(loop_runs):
    _con, runs = loop_runs
    for se, sg in zip(runs["eager"], runs["graph"]):
        assert se[0] == sg[0]
        for k in (1, 2, 3):
            assert torch.equal(se[k], sg[k]), f"t={se[0]} state {k}"


def test_loop_torch_noise(model):
    """noise="torch" under the captured step: completes, holds the known entries, and leaves the CPU generator
    where the unconstrained run leaves it (the replacement's noise is device Philox)."""
    cond, null = C.conditioning(1)
    con = loop_constraint()
    after, last = [], []
    for c in (con, None):
        torch.manual_seed(4321)
        for s in model.sample_states(LOOP_NAT, None, 2.0, 1e-5, noise="torch", seed=31, text_embeds=cond,
                                     null_text_embeds=null, clone=False, constraint=c):
            pass
        torch.cuda.synchronize()
        last.append(tuple(v.clone() if torch.is_tensor(v) else v for v in s))
        after.append(torch.get_rng_state())
    assert last[0][0] == 0
    held_ok(last[0], con)
    assert torch.equal(after[0], after[1])
    for rows in (slice(6, 12), slice(18, 24)):  # the unconstrained crystals keep the reference's stream
        assert torch.equal(last[0][2][rows], last[1][2][rows])


def test_sample_with_a_formula(model):
    cond, null = C.conditioning(1)
    atoms = model.sample("TiO2", n_atoms=6, n_samples=4, constraint=Constraint.from_formula("TiO2", 6, 4),
                         noise="philox", seed=3, text_embeds=cond, null_text_embeds=null)
    assert len(atoms) == 4
    for at in atoms:
        assert sorted(int(z) for z in at.numbers) == [8, 8, 8, 8, 22, 22]


def test_lanes_and_foreign_batches_are_refused(model):
    cond, null = C.conditioning(1)
    con = Constraint.from_formula("TiO2", 6, 4)
    with pytest.raises(ValueError, match="lanes"):
        next(model.sample_states(LOOP_NAT, None, noise="philox", text_embeds=cond, null_text_embeds=null, lanes=2,
                                 constraint=con))
    with pytest.raises(ValueError, match="crystals"):
        next(model.sample_states([6, 6], None, noise="philox", text_embeds=cond, null_text_embeds=null,
                                 constraint=con))
