"""The training forward's kernels (k_train_noise, k_train_lattice, k_train_node_loss, k_train_reduce;
csrc/kernels.hip) through chm_debug_train_update, which runs them with chm_training_loss's own arguments on
caller-supplied decoder outputs, against the CPU reference of tests/train_cases.py (pinned to the oracle by
tests/test_train_cases.py).

x_t atom types are the float64 decisions on every node (the seeds leave no near tie: test_every_node_counts); x_t
coordinates and l_t equal the float32 restatement BIT FOR BIT. The score target, the per-node KL and cross entropy
and the six outputs are measured against float64: per quantity the device may take 16 times the largest error the
float32 restatement itself makes against float64 over all cases of this file (the margin of the step and the dedup
tests; the baselines are computed here, none is fixed in advance). Each comparison prints its figures before it
asserts (pytest -s); the table is in profiles/r13/train_unit/README.md.

Guards: sentinel rows behind every output must stay untouched. A HIP error from the hook ends the session: nothing
else runs on the device after a fault. Run on an MI355X: pytest -m gpu."""

import ctypes

import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict
from oracle import chemeleon_oracle as O

from . import train_cases as C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
SENTINEL_ROWS = 8
SENT_A, SENT_F = -7777, -123.25
MARGIN = 16
CASES = [pytest.param(n, T, A, id=f"{n}-T{T}-A{A}") for n, _nat, T, A in C.cases()]


@pytest.fixture(scope="module")
def decoders():
    """A -> a one-layer decoder of A classes with synthetic weights (time-conditioned, no text)."""
    from chemeleon_amd.modules.cspnet import CSPNet
    cache = {}

    def get(A):
        if A not in cache:
            cfg = dict(default_config(), max_atoms=A, num_layers=1, text_dim=0)
            net = CSPNet(hidden_dim=cfg["hidden_dim"], time_dim=cfg["time_dim"], text_dim=0, num_layers=1, max_atoms=A,
                         act_fn=cfg["act_fn"], dis_emb=cfg["dis_emb"], num_freqs=cfg["num_freqs"],
                         edge_style=cfg["edge_style"], cutoff=cfg["cutoff"], max_neighbors=cfg["max_neighbors"],
                         ln=cfg["ln"], ip=cfg["ip"], smooth=cfg["smooth"], pred_atom_types=cfg["pred_atom_types"])
            net.load_state_dict(synthetic_state_dict(cfg))
            cache[A] = net.to(DEV).eval()
        return cache[A]

    return get


@pytest.fixture(scope="module")
def world():
    """Per (T, A): the device tables, and per (shape, k) the inputs with their float64 and float32 chains. The
    baselines need every case before the first assertion, so everything is computed once, on the CPU."""
    w = {"tables": {}, "cases": {}, "base": {q: 0.0 for q in C.QUANTITIES}}
    for name, _nat, T, A in C.cases():
        ref = C.ref_model(T, A)
        if (T, A) not in w["tables"]:
            keep = [v.contiguous().to(DEV) for v in (C.coef_table(ref), ref.q_one_step, ref.q_mats)]
            tt = _lib.chm_train_tables(T, _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]),
                                       C.WEIGHTS["d3pm_hybrid_coeff"], C.WEIGHTS["cost_atom_types"],
                                       C.WEIGHTS["cost_lattice"], C.WEIGHTS["cost_coords"])
            w["tables"][T, A] = (tt, keep)
        for k in C.ROTATIONS[name]:
            d = C.inputs(name, T, A, k)
            r64, r32 = C.reference(ref, d, torch.float64), C.reference(ref, d, torch.float32)
            e = C.errors(r32, r64, d)
            for q in C.QUANTITIES:
                w["base"][q] = max(w["base"][q], e[q])
            w["cases"][name, T, A, k] = (d, r64, r32, e)
    print("float32 restatement against float64, largest error per quantity: " +
          ", ".join(f"{q} {v:.3e}" for q, v in w["base"].items()))
    return w


@pytest.fixture(scope="module")
def batches(decoders):
    cache = {}

    def get(A, nat):
        key = (A, tuple(nat))
        if key not in cache:
            cache[key] = decoders(A).hip_batch(list(nat), max_pairs=1, private=True)
        return cache[key]

    return get


def padded(shape, dtype, rows, fill):
    return torch.full((shape[0] + rows,) + tuple(shape[1:]), fill, dtype=dtype, device=DEV)


def hook(b, tt, d, A, heads=None):
    """One chm_debug_train_update call on device copies of d's inputs (heads = (types, coords, lattice) device
    tensors instead of d's), every output with sentinel rows behind it. Returns the outputs on the CPU."""
    lib = _lib.load()
    N, B = d["a0"].shape[0], d["t"].shape[0]
    assert int(d["a0"].min()) >= 0 and int(d["a0"].max()) < A and int(d["t"].min()) >= 1 and int(d["t"].max()) <= tt.T
    nl = (d["nl"] * O.LATTICE_MASK).float()
    dv = {k: d[k].to(DEV).contiguous() for k in ("t", "a0", "x0", "l0", "ra", "nx")}
    nl = nl.to(DEV).contiguous()
    ty, co, la = heads if heads is not None else [d[k].to(DEV).float().contiguous() for k in ("types", "coords", "lattice")]
    out = padded((6,), torch.float32, SENTINEL_ROWS, SENT_F)
    a_t = padded((N,), torch.long, SENTINEL_ROWS, SENT_A)
    x_t, tg = padded((N, 3), torch.float32, SENTINEL_ROWS, SENT_F), padded((N, 3), torch.float32, SENTINEL_ROWS, SENT_F)
    l_t = padded((B, 3, 3), torch.float32, SENTINEL_ROWS, SENT_F)
    part = padded((N, 2), torch.float32, SENTINEL_ROWS, SENT_F)
    P = _lib.ptr
    rc = lib.chm_debug_train_update(b.handle, ctypes.byref(tt), P(dv["t"]), P(dv["a0"]), P(dv["x0"]), P(dv["l0"]),
                                    P(dv["ra"]), P(nl), P(dv["nx"]), P(ty), ty.numel(), P(co), co.numel(), P(la),
                                    la.numel(), P(out), P(a_t), P(x_t), P(l_t), P(tg), P(part), _lib.stream_handle())
    if rc == -2:  # CHM_E_HIP: nothing else runs on the device after a fault
        pytest.exit(f"chm_debug_train_update: {lib.chm_last_error().decode(errors='replace')}", returncode=3)
    assert rc == 0, lib.chm_last_error()
    out, a_t, x_t, tg, l_t, part = (v.cpu() for v in (out, a_t, x_t, tg, l_t, part))
    assert bool((out[6:] == SENT_F).all()) and bool((a_t[N:] == SENT_A).all()) and bool((x_t[N:] == SENT_F).all()) and \
        bool((tg[N:] == SENT_F).all()) and bool((l_t[B:] == SENT_F).all()) and bool((part[N:] == SENT_F).all()), \
        "rows behind an output were written"
    got = {"a_t": a_t[:N], "x_t": x_t[:N], "l_t": l_t[:B], "target": tg[:N], "kl": part[:N, 0], "ce": part[:N, 1],
           "out": out[:6]}
    got.update({q: out[i] for i, q in enumerate(C.OUT_NAMES)})
    return got


def same_bits(got, want, what):
    """Bit equality, after printing how far apart the two are; returns the verdict."""
    eq = torch.equal(C.bits(got), C.bits(want))
    if eq:
        print(f"{what}: bit-identical")
    else:
        fin = torch.isfinite(got) & torch.isfinite(want)
        u = C.ulps(got[fin], want[fin])
        print(f"{what}: {int((C.bits(got) != C.bits(want)).sum())} of {got.numel()} elements differ, max "
              f"{int(u.max()) if u.numel() else -1} ulp, non-finite mismatches {int((~fin).sum())}")
    return eq


# ------------------------------------------------------------------------------------------ the noised state
@pytest.mark.parametrize("name,T,A", CASES)
def test_noised_state(world, batches, name, T, A):
    """k_train_noise and k_train_lattice: x_t atom types are the float64 decisions on every node, the first of two
    infinite scores included; x_t coordinates (the wrap edges among them) and l_t equal the restatement bit for bit."""
    tt, _keep = world["tables"][T, A]
    bad = []
    for k in C.ROTATIONS[name]:
        d, r64, r32, _e = world["cases"][name, T, A, k]
        got = hook(batches(A, C.SHAPES[name]), tt, d, A)
        what = f"{name} T {T} A {A} k {k}"
        assert torch.equal(got["a_t"], r64["a_t"]), f"{what}: {int((got['a_t'] != r64['a_t']).sum())} atom types differ"
        assert bool(torch.isfinite(got["x_t"]).all()) and bool(torch.isfinite(got["l_t"]).all())
        ok_l = same_bits(got["l_t"], r32["l_t"], f"{what} l_t")
        ok_x = same_bits(got["x_t"], r32["x_t"], f"{what} x_t")
        if not (ok_l and ok_x):
            bad.append((k, "l_t" if not ok_l else "", "x_t" if not ok_x else ""))
    assert not bad, f"{name} T {T} A {A}: differs from the float32 restatement at (k, tensors) {bad}"


# ------------------------------------------------------------------------------------------ the losses
@pytest.mark.parametrize("name,T,A", CASES)
def test_losses_against_float64(world, batches, name, T, A):
    """The score target (directly where sqrt(sigma_norm) >= 1e-2, elsewhere through its numerator), the per-node KL
    and cross entropy and the six outputs, each within MARGIN x the float32 restatement's largest error; and the six
    outputs among themselves: loss_atom_types = vb + hybrid ce, loss the weighted sum, the coordinate MSE over the
    device's own target, the lattice MSE over 6 entries per crystal."""
    tt, _keep = world["tables"][T, A]
    base = world["base"]
    nat = C.SHAPES[name]
    B, N = len(nat), sum(nat)
    fails = []
    for k in C.ROTATIONS[name]:
        d, r64, _r32, e32 = world["cases"][name, T, A, k]
        got = hook(batches(A, nat), tt, d, A)
        what = f"{name} T {T} A {A} k {k}"
        assert torch.equal(got["a_t"], r64["a_t"]), what
        assert all(bool(torch.isfinite(got[q]).all()) for q in ("target", "kl", "ce", "out")), f"{what}: not finite"
        e = C.errors(got, r64, d)
        print(f"{what}: " + ", ".join(f"{q} device {e[q]:.3e} float32 {e32[q]:.3e}" for q in C.QUANTITIES))
        fails += [f"{what} {q}: {e[q]:.3e} against {MARGIN} x {base[q]:.3e}" for q in C.QUANTITIES if e[q] > MARGIN * base[q]]
        # the six outputs among themselves (float64 from the device's own values); bounds: a sum of n non-negative
        # fp32 terms, each with a few roundings of its own, is within (n + 8) 2^-24 of the exact sum, relatively
        o = got["out"].double()
        h, ca, cl, cx = (C.WEIGHTS[q] for q in ("d3pm_hybrid_coeff", "cost_atom_types", "cost_lattice", "cost_coords"))
        u = 2.0 ** -23
        assert abs(float(o[3] - (o[1] + h * o[2]))) <= 2 * u * float(o[1].abs() + h * o[2].abs()), f"{what}: loss_atom_types"
        assert abs(float(o[0] - (ca * o[3] + cl * o[4] + cx * o[5]))) <= 4 * u * float(ca * o[3].abs() + cl * o[4] + cx * o[5]), f"{what}: loss"
        vb, ce = got["kl"].double().mean(), got["ce"].double().mean()
        assert abs(float(o[1] - vb)) <= (N + 8) * u / 2 * float(got["kl"].double().abs().mean()), f"{what}: vb_loss is the mean"
        assert abs(float(o[2] - ce)) <= (N + 8) * u / 2 * float(got["ce"].double().abs().mean()), f"{what}: ce_loss is the mean"
        lx = float(((d["coords"].double() - got["target"].double()) ** 2).mean())
        assert abs(float(o[5]) - lx) <= (3 * N + 8) * u / 2 * lx, f"{what}: loss_coords {float(o[5])} against {lx}"
        nl = (d["nl"] * O.LATTICE_MASK).double()
        ll = float(((d["lattice"].double() - nl) ** 2).masked_select(O.LATTICE_MASK).sum()) / (6 * B)
        assert abs(float(o[4]) - ll) <= (9 * B + 8) * u / 2 * ll, f"{what}: loss_lattice {float(o[4])} against {ll}"
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ a crystal alone
@pytest.mark.parametrize("A", (5, 104))
def test_crystal_alone(world, batches, A):
    """Crystal 1 of the ragged batch alone gives the bits it gives inside the batch: the noised state, the score
    target and the per-node partials."""
    T = 100
    tt, _keep = world["tables"][T, A]
    d = world["cases"]["ragged", T, A, 0][0]
    nat = C.SHAPES["ragged"]
    whole = hook(batches(A, nat), tt, d, A)
    g, n0, n1 = 1, nat[0], nat[0] + nat[1]
    one = {k: d[k][n0:n1] for k in ("a0", "x0", "ra", "nx", "types", "coords")}
    one.update({k: d[k][g:g + 1] for k in ("t", "l0", "nl", "lattice")})
    alone = hook(batches(A, [nat[g]]), tt, one, A)
    assert torch.equal(alone["a_t"], whole["a_t"][n0:n1])
    for q in ("x_t", "target", "kl", "ce"):
        assert torch.equal(C.bits(alone[q]), C.bits(whole[q][n0:n1])), q
    assert torch.equal(C.bits(alone["l_t"]), C.bits(whole["l_t"][g:g + 1]))


# ------------------------------------------------------------------------------------------ the hook is the forward
@pytest.mark.parametrize("A", (5, 104))
def test_hook_is_the_training_forward(world, decoders, batches, A):
    """chm_training_loss against chm_decoder_forward on the noised state it returned and the hook on those heads: the
    six outputs and the noised state bit-identical."""
    lib = _lib.load()
    T = 100
    tt, _keep = world["tables"][T, A]
    d = world["cases"]["ragged", T, A, 0][0]
    nat = C.SHAPES["ragged"]
    B, N = len(nat), sum(nat)
    net, b = decoders(A), batches(A, nat)
    P, st = _lib.ptr, _lib.stream_handle()
    dv = {k: d[k].to(DEV).contiguous() for k in ("t", "a0", "x0", "l0", "ra", "nx")}
    nl = (d["nl"] * O.LATTICE_MASK).float().to(DEV).contiguous()
    te = O.time_embedding(d["t"], net.time_dim).float().to(DEV).contiguous()
    out, a_t = torch.empty(6, device=DEV), torch.empty(N, dtype=torch.long, device=DEV)
    x_t, tg, l_t = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV), torch.empty(B, 3, 3, device=DEV)
    _lib.check(lib.chm_training_loss(b.handle, ctypes.byref(tt), P(dv["t"]), P(dv["a0"]), P(dv["x0"]), P(dv["l0"]), P(te),
                                     None, P(dv["ra"]), P(nl), P(dv["nx"]), P(out), P(a_t), P(x_t), P(l_t), P(tg), None,
                                     None, st), "chm_training_loss")
    torch.cuda.synchronize()
    ty, la, co = torch.empty(N, A, device=DEV), torch.empty(B, 3, 3, device=DEV), torch.empty(N, 3, device=DEV)
    _lib.check(lib.chm_decoder_forward(b.handle, 1, P(a_t), P(x_t), P(l_t), P(te), net.time_dim, None, P(ty), P(la),
                                       P(co), None, st), "chm_decoder_forward")
    torch.cuda.synchronize()
    got = hook(b, tt, d, A, heads=(ty, co, la))
    assert torch.equal(got["a_t"], a_t.cpu())
    for q, w in (("x_t", x_t), ("l_t", l_t), ("target", tg), ("out", out)):
        assert torch.equal(C.bits(got[q]), C.bits(w.cpu())), q
    assert bool(torch.isfinite(got["out"]).all())


# ------------------------------------------------------------------------------------------ refusals on a real batch
def test_hook_refuses_what_the_batch_cannot_take(world, batches):
    lib = _lib.load()
    A, T = 104, 100
    tt, _keep = world["tables"][T, A]
    nat = C.SHAPES["ragged"]
    B, N = len(nat), sum(nat)
    b = batches(A, nat)
    z = torch.zeros(N * A, device=DEV)
    zi = torch.ones(N, dtype=torch.long, device=DEV)
    outs = [torch.zeros(6, device=DEV), torch.zeros(N, dtype=torch.long, device=DEV), torch.zeros(N, 3, device=DEV),
            torch.zeros(B, 3, 3, device=DEV), torch.zeros(N, 3, device=DEV), torch.zeros(N, 2, device=DEV)]
    P = _lib.ptr

    def call(n_types=N * A, n_coords=3 * N, n_lattice=9 * B):
        return lib.chm_debug_train_update(b.handle, ctypes.byref(tt), P(zi), P(zi), P(z), P(z), P(z), P(z), P(z), P(z),
                                          n_types, P(z), n_coords, P(z), n_lattice, *[P(v) for v in outs],
                                          _lib.stream_handle())

    assert call(n_types=2 * N * A) == -1 and b"n_types" in lib.chm_last_error()
    assert call(n_coords=3 * N - 3) == -1 and b"n_coords" in lib.chm_last_error()
    assert call(n_lattice=9) == -1 and b"n_lattice" in lib.chm_last_error()
    torch.cuda.synchronize()
    assert all(bool((v == 0).all()) for v in outs)  # (nothing ran)
    assert call() == 0, lib.chm_last_error()
