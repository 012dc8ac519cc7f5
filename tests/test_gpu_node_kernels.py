"""The decoder's node-side kernels (k_cond_in, k_embed with its folded per-graph terms and cleared words, k_graph_bias,
k_film_ln, k_layer_norm, k_graph_heads, k_split_heads, store_split_row512; csrc/kernels.hip) through
chm_debug_node_stage, which runs them by the functions a decoder call runs them with, against the CPU reference of
tests/node_cases.py (pinned to cspnet.py's modules and to the oracle by tests/test_node_cases.py).

Copies (cin, Hres after the embedding, types, coords) are compared BIT FOR BIT. Arithmetic (the per-graph terms,
Hres / Hl after FiLM + LayerNorm, Hf, LAT) is measured against float64 with test_gpu_parity.scaled_err: per quantity
the device may take 16 times the largest error the float32 restatement itself makes against float64 over all cases of
this file (the margin of the step, train and dedup tests; the baselines are computed here, none is fixed in advance).
The rows of kind big_mean (1e4 + 1e-2 randn: their LayerNorm loses 4 digits in fp32 whatever the order) and the
lattice outputs of crystals holding one are quantities of their own ("...@big_mean"), so that they do not widen the
bound of every other row. A constant row gives the LayerNorm bias bit for bit. The derived outputs (row maxima,
packed chunk exponents, split rows and their layout) are exact functions of the kernel's own fp32 output and are
compared bit for bit with numpy. Each comparison prints its figures before it asserts (pytest -s); the table is in
profiles/r15/node_unit/README.md.

Guards: sentinel elements behind every output must stay untouched. A HIP error from the hook ends the session:
nothing else runs on the device after a fault. Run on an MI355X: pytest -m gpu."""

import ctypes
import time

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from oracle import chemeleon_oracle as O

from . import node_cases as C
from .test_gpu_parity import close, scaled_err

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
PAD = 8 * C.H  # sentinel elements behind every output (8 rows of the widest)
SENT_F, SENT_I, PATTERN = -123.25, -7777, 0x5A5A5A5A
MARGIN = 16
H, TD = C.H, C.TD
CASES = [pytest.param(n, P, id=f"{n}-P{P}") for n, P in C.cases()]
PLANS = {"f32": ("f32", 0), "split16": ("split16", 0), "split16_ps": ("split16", 1)}
# (model, layer) of the stage-3 runs; the baselines cover every one of them
LAYERS = (("a", 0), ("a", 1), ("b", 32), ("c", 0))
BASE_MODELS = ("a", "b", "c")
MEASURED = {}  # quantity -> largest device error seen (printed by the last test)


@pytest.fixture(scope="module")
def nets():
    """model name -> the CSPNet on the device (built on first use; (b)'s creation time is printed)."""
    from .test_node_cases import net_of
    cache = {}

    def get(model):
        if model not in cache:
            net = net_of(model).to(DEV).eval()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net.hip_model()
            torch.cuda.synchronize()
            print(f"model ({model}): {C.MODELS[model]['num_layers']} layers, chm_model_create {time.perf_counter() - t0:.2f} s")
            # every fc case on the pair grid (both edge layers in one launch): the plan whose embedding launch clears
            # the grid's words. The node-side results do not depend on it.
            net.set_option("edge_layer_min", 1)
            net.set_option("edge_rows_short", 0)
            cache[model] = net
        return cache[model]

    return get


@pytest.fixture(scope="module")
def batches(nets):
    cache = {}

    def get(model, name, P, plan):
        """The batch of (model, case, plan), the model left in that plan's math mode and options."""
        net = nets(model)
        math, ps = PLANS[plan]
        if net.get_math() != math:
            net.set_math(math)
        net.set_option("node_ps", ps)
        key = (model, name, P, plan)
        if key not in cache:
            cache[key] = net.hip_batch(C.SHAPES[name], max_pairs=P, private=True)
        return cache[key]

    return get


def errs(got, ref, mask=None):
    """(error of the rows outside mask, error of the rows inside it); mask over the leading axes of ref."""
    e = scaled_err(got, ref)
    if mask is None or not mask.any():
        return float(e.max()), 0.0
    return (float(e[~mask].max()) if (~mask).any() else 0.0), float(e[mask].max())


@pytest.fixture(scope="module")
def world():
    """Per (model, case): the inputs, and per stage the float64 and float32 results with the restatement's errors.
    The baselines need every case before the first assertion, so everything is computed once, on the CPU."""
    w = {"in": {}, "gbias": {}, "film": {}, "tail": {}, "base": {}}

    def note(q, e):
        for k, v in zip((q, q + "@big_mean"), e):
            w["base"][k] = max(w["base"].get(k, 0.0), v)

    for model in BASE_MODELS:
        sd, L = C.state_dict(model), C.MODELS[model]["num_layers"]
        film = model != "c"
        for name, P in C.cases():
            d = C.inputs(name, P, model)
            w["in"][model, name, P] = d
            rows, graphs = C.kind_mask(name, P, "big_mean"), C.graph_mask(name, P, "big_mean")
            g64 = C.graph_bias64(sd, L, d["lat"]).numpy()
            w["gbias"][model, name, P] = g64
            note("gbias", errs(C.graph_bias32(sd, L, d["lat"]), g64))
            for m2, layer in LAYERS:
                if m2 == model:
                    r64 = [v.numpy() for v in C.film_ln64(sd, layer, d, P, film)]
                    r32 = C.film_ln32(sd, layer, d, P, film)
                    w["film"][model, layer, name, P] = r64
                    note("Hres", errs(r32[0], r64[0], rows))
                    note("Hl", errs(r32[1], r64[1], rows))
            t64 = [v.numpy() for v in C.tail64(sd, d, P)]
            t32 = C.tail32(sd, d, P)
            w["tail"][model, name, P] = t64
            note("Hf", errs(t32[0], t64[0], rows))
            note("LAT", errs(t32[1], t64[1], graphs))
    print("float32 restatement against float64, largest error per quantity: " +
          ", ".join(f"{q} {v:.3e}" for q, v in sorted(w["base"].items())))
    return w


def measure(world, q, e, what, fails):
    for k, v in zip((q, q + "@big_mean"), e):
        b = world["base"][k]
        MEASURED[k] = max(MEASURED.get(k, 0.0), v)
        print(f"{what} {k}: device {v:.3e}, float32 {b:.3e}, ratio {v / b if b else 0.0:.2f}")
        if v > MARGIN * b:
            fails.append(f"{what} {k}: {v:.3e} against {MARGIN} x {b:.3e}")


# ------------------------------------------------------------------------------------------ the hook
def run(b, pairs, stage, layer=0, ins=None, outs=None, inouts=None, tstride=0, expect=0):
    """One chm_debug_node_stage call. ins: field -> tensor (CPU or device); outs: field -> (elements, dtype); inouts:
    field -> CPU tensor written behind the call as well. Every output has PAD sentinel elements behind it, which must
    stay untouched. Returns field -> numpy array (flat)."""
    lib = _lib.load()
    io = _lib.chm_debug_node_io()
    io.tstride = tstride
    keep, bufs = [], {}
    for k, t in (ins or {}).items():
        t = t.to(DEV).contiguous()
        keep.append(t)
        setattr(io, "d_" + k, t.data_ptr())
        setattr(io, "n_" + k, t.numel())
    for k, (n, dt) in (outs or {}).items():
        bufs[k] = (torch.full((n + PAD,), SENT_I if dt in (torch.int32, torch.int64) else SENT_F, dtype=dt, device=DEV), n)
    for k, t in (inouts or {}).items():
        buf = torch.full((t.numel() + PAD,), SENT_I if t.dtype == torch.int32 else SENT_F, dtype=t.dtype, device=DEV)
        buf[:t.numel()] = t.reshape(-1).to(DEV)
        bufs[k] = (buf, t.numel())
    for k, (buf, n) in bufs.items():
        setattr(io, "d_" + k, buf.data_ptr())
        setattr(io, "n_" + k, n)
    torch.cuda.synchronize()
    rc = lib.chm_debug_node_stage(b.handle, pairs, stage, layer, ctypes.byref(io), _lib.stream_handle())
    if rc == -2:  # CHM_E_HIP: nothing else runs on the device after a fault
        pytest.exit(f"chm_debug_node_stage: {lib.chm_last_error().decode(errors='replace')}", returncode=3)
    assert rc == expect, (rc, lib.chm_last_error())
    got = {}
    for k, (buf, n) in bufs.items():
        host = buf.cpu()
        sent = SENT_I if host.dtype in (torch.int32, torch.int64) else SENT_F
        assert bool((host[n:] == sent).all()), f"stage {stage}: elements behind {k} were written"
        got[k] = host[:n].numpy()
    return got


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want).reshape(np.shape(got))
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = got.view(u) != want.view(u)
    print(f"{what}: " + ("bit-identical" if not diff.any() else f"{int(diff.sum())} of {diff.size} elements differ"))
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ, first at {np.argwhere(diff)[0].tolist()}"


def check_split(split, words, rows, what):
    """The split rows and packed exponents of fp32 rows [R, H] (the kernel's own output) against the numpy model."""
    raw, ex = C.split_rows(rows.reshape(-1, H))
    same_bits(words, ex, f"{what} chunk exponents")
    same_bits(split.reshape(-1, 2 * H), raw, f"{what} split rows [H/16][hi 16 | lo 16]")


# ------------------------------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("model", ["a", "b"])
@pytest.mark.parametrize("name,P", CASES)
def test_cond_in(world, batches, model, name, P):
    """k_cond_in: cin = [time row | text row of conditioning c], bit for bit, in its three forms: a time table read
    at the device's t, the same row per graph at stride time_dim, and differing per-graph rows."""
    d = world["in"][model, name, P]
    b = batches(model, name, P, "split16")
    X = C.MODELS[model]["text_dim"]
    B = len(d["natoms"])
    text = {"text0": d["text"][0]} if X else {}
    if X and P == 2:
        text["text1"] = d["text"][1]
    out = {"cin": (P * B * (TD + X), torch.float32)}
    want = C.cond_in(d, P, X).numpy()
    by_t = run(b, P, 1, ins=dict(text, temb=d["table"], t=torch.tensor([d["t"]], dtype=torch.int32)), outs=out)["cin"]
    same_bits(by_t, want, f"{model} {name} P {P} cin (device t)")
    by_row = run(b, P, 1, ins=dict(text, temb=d["temb"]), outs=out, tstride=TD)["cin"]
    same_bits(by_row, by_t, f"{model} {name} P {P} cin (per-graph stride) against the device-t form")
    rows = run(b, P, 1, ins=dict(text, temb=d["temb_rows"]), outs=out, tstride=TD)["cin"]
    same_bits(rows, C.cond_in(d, P, X, tstride_rows=True).numpy(), f"{model} {name} P {P} cin (differing rows)")
    one = run(b, P, 1, ins=dict(text, temb=d["temb"][:1]), outs=out, tstride=0)["cin"]
    same_bits(one, want, f"{model} {name} P {P} cin (stride 0)")


# ------------------------------------------------------------------------------------------ stage 2
@pytest.mark.parametrize("model,plan", [("a", "f32"), ("a", "split16"), ("a", "split16_ps"), ("b", "split16"),
                                        ("c", "split16"), ("c", "split16_ps")])
@pytest.mark.parametrize("name,P", CASES)
def test_embed_and_graph_bias(world, batches, model, plan, name, P):
    """k_embed and k_graph_bias: Hres = the embedding rows bit for bit for every conditioning; the per-graph terms of
    ALL layers against float64; the row maxima / the split rows and exponents exact in the kernel's own rows; on the
    pair grid the launch's cleared words all zero and the words behind them untouched."""
    lib = _lib.load()
    d = world["in"][model, name, P]
    b = batches(model, name, P, plan)
    sd, L = C.state_dict(model), C.MODELS[model]["num_layers"]
    B, N = len(d["natoms"]), sum(d["natoms"])
    R = P * N
    what = f"{model} {plan} {name} P {P}"
    outs = {"Hres": (R * H, torch.float32), "gbias": (L * B * H, torch.float32)}
    if plan == "split16":
        outs["rmax"] = (R, torch.float32)
    if plan == "split16_ps":
        outs["split"], outs["exp"] = (R * 2 * H, torch.float16), (R, torch.int32)
    inouts = {}
    ncl = ctypes.c_int64()
    nfl = int(lib.chm_debug_node_flag_words(b.handle, P, ctypes.byref(ncl)))
    if plan == "f32":
        assert nfl == 0
    else:
        assert nfl > 0 and 128 < ncl.value <= nfl, f"{what}: not on the pair grid ({nfl} flag words)"
        inouts["flags"] = torch.full((nfl,), PATTERN, dtype=torch.int32)
    got = run(b, P, 2, ins={"a": d["a"], "lat": d["lat"]}, outs=outs, inouts=inouts)
    emb = sd["node_embedding.weight"].numpy()[d["a"].numpy()]
    hres = got["Hres"].reshape(P, N, H)
    same_bits(hres, np.broadcast_to(emb, (P, N, H)), f"{what} Hres")
    assert np.isfinite(got["gbias"]).all(), f"{what}: a per-graph term was not written"
    fails = []
    measure(world, "gbias", errs(got["gbias"].reshape(L, B, H), world["gbias"][model, name, P]), what, fails)
    for l0 in range(0, L, C.GB_LAYERS):  # (per launch group, so that a misplaced group is named)
        e = errs(got["gbias"].reshape(L, B, H)[l0:l0 + C.GB_LAYERS], world["gbias"][model, name, P][l0:l0 + C.GB_LAYERS])[0]
        if e > MARGIN * world["base"]["gbias"]:
            fails.append(f"{what} gbias layers {l0}..: {e:.3e}")
    if "rmax" in got:
        same_bits(got["rmax"], C.row_max(hres), f"{what} rmax")
    if "split" in got:
        check_split(got["split"], got["exp"], hres, f"{what} Hres")
    if inouts:
        fl = got["flags"]
        assert (fl[:ncl.value] == 0).all(), f"{what}: {int((fl[:ncl.value] != 0).sum())} of the launch's words not cleared"
        assert (fl[ncl.value:] == PATTERN).all(), f"{what}: words behind the cleared range were written"
        print(f"{what}: {ncl.value} words cleared, {nfl - ncl.value} guard words behind them untouched")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ stage 3
@pytest.mark.parametrize("model,layer,plan", [("a", 0, "f32"), ("a", 1, "split16"), ("a", 0, "split16_ps"),
                                              ("b", 32, "split16"), ("c", 0, "f32"), ("c", 0, "split16"),
                                              ("c", 0, "split16_ps")])
@pytest.mark.parametrize("name,P", CASES)
def test_film_layer_norm(world, batches, model, layer, plan, name, P):
    """k_film_ln: the residual stream after FiLM and the layer's LayerNorm against float64 (film-less: Hres unchanged
    bit for bit, a constant row's LayerNorm its bias bit for bit); the four row-max rows and Hl's split rows exact."""
    d = world["in"][model, name, P]
    b = batches(model, name, P, plan)
    sd = C.state_dict(model)
    film = model != "c"
    N = sum(d["natoms"])
    R = P * N
    what = f"{model} layer {layer} {plan} {name} P {P}"
    ins = {"Y": d["Y"][:P], "cemb": d["cemb"][:P]} if film else {}
    outs = {"Hl": (R * H, torch.float32)}
    if plan == "split16":
        outs["rmax"] = (4 * R, torch.float32)
    if plan == "split16_ps":
        outs["split"], outs["exp"] = (R * 2 * H, torch.float16), (R, torch.int32)
    got = run(b, P, 3, layer, ins=ins, outs=outs, inouts={"Hres": d["Hres"][:P].contiguous()})
    hres, hl = got["Hres"].reshape(P, N, H), got["Hl"].reshape(P, N, H)
    assert np.isfinite(hres).all() and np.isfinite(hl).all(), f"{what}: not finite"
    r64 = world["film"][model, layer, name, P]
    rows = C.kind_mask(name, P, "big_mean")
    fails = []
    if film:
        measure(world, "Hres", errs(hres, r64[0], rows), what, fails)
    else:
        same_bits(hres, d["Hres"][:P].numpy(), f"{what} Hres (no FilmLayer)")
        const = C.kind_mask(name, P, "const")
        lb = sd[f"csp_layer_{layer}.layer_norm.bias"].numpy()
        same_bits(hl[const], np.broadcast_to(lb, hl[const].shape), f"{what} Hl of {int(const.sum())} constant rows")
    measure(world, "Hl", errs(hl, r64[1], rows), what, fails)
    if "rmax" in got:
        rmx = got["rmax"].reshape(4, R)
        same_bits(rmx[1], C.row_max(hl), f"{what} rmx[RMX_HL]")
        assert (rmx[[0, 2, 3]].view(np.uint32) == 0).all(), f"{what}: rmx rows H / AGG / U are not +0"
    if "split" in got:
        check_split(got["split"], got["exp"], hl, f"{what} Hl")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ stage 4
@pytest.mark.parametrize("model", ["a", "c", "d1", "d125"])
@pytest.mark.parametrize("name,P", CASES)
def test_tail(world, batches, model, name, P):
    """k_layer_norm, k_graph_heads, k_split_heads: Hf and LAT against float64, a constant row's Hf the bias bit for
    bit; types and coords copied bit for bit, each also with the other NULL."""
    base = "a" if model.startswith("d") else model  # ((d) differs from (a) in the class count alone)
    d = world["in"][base, name, P]
    b = batches(model, name, P, "split16")
    sd, A = C.state_dict(base), C.MODELS[model]["max_atoms"]
    B, N = len(d["natoms"]), sum(d["natoms"])
    R = P * N
    what = f"{model} {name} P {P}"
    ins = {"Hres": d["Hres"][:P], "lat": d["lat"], "HO": d["HO"][:R]}
    f32 = torch.float32
    outs = {"Hf": (R * H, f32), "LAT": (P * B * 9, f32), "types": (R * A, f32), "coords": (R * 3, f32)}
    got = run(b, P, 4, ins=ins, outs=outs)
    ty, co = C.split_heads(d, P, A)
    same_bits(got["types"], ty.numpy(), f"{what} types")
    same_bits(got["coords"], co.numpy(), f"{what} coords")
    for drop in ("types", "coords"):
        part = run(b, P, 4, ins=ins, outs={k: v for k, v in outs.items() if k != drop})
        for k in part:
            same_bits(part[k], got[k], f"{what} {k} without {drop}")
    hf, lat = got["Hf"].reshape(P, N, H), got["LAT"].reshape(P, B, 3, 3)
    assert np.isfinite(hf).all() and np.isfinite(lat).all(), f"{what}: not finite"
    const = C.kind_mask(name, P, "const")
    flb = sd["final_layer_norm.bias"].numpy()
    same_bits(hf[const], np.broadcast_to(flb, hf[const].shape), f"{what} Hf of {int(const.sum())} constant rows")
    t64 = world["tail"][base, name, P]
    fails = []
    measure(world, "Hf", errs(hf, t64[0], C.kind_mask(name, P, "big_mean")), what, fails)
    measure(world, "LAT", errs(lat, t64[1], C.graph_mask(name, P, "big_mean")), what, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ refusals on a real batch
def test_hook_refuses_what_the_plan_does_not_write(world, batches):
    lib = _lib.load()
    name, P = "123", 2
    d = world["in"]["a", name, P]
    B, N = len(d["natoms"]), sum(d["natoms"])
    R, L = P * N, 2
    f32 = torch.float32
    s2 = {"Hres": (R * H, f32), "gbias": (L * B * H, f32)}
    s3 = {"Hl": (R * H, f32)}
    rmax2, rmax3 = {"rmax": (R, f32)}, {"rmax": (4 * R, f32)}
    split = {"split": (R * 2 * H, torch.float16), "exp": (R, torch.int32)}
    ins2 = {"a": d["a"], "lat": d["lat"]}
    ins3 = {"Y": d["Y"], "cemb": d["cemb"]}
    hres = {"Hres": d["Hres"].contiguous()}

    def refused(plan, stage, extra, field):
        b = batches("a", name, P, plan)
        if stage == 2:
            run(b, P, 2, ins=ins2, outs=dict(s2, **extra), expect=-1)
        else:
            run(b, P, 3, ins=ins3, outs=dict(s3, **extra), inouts=hres, expect=-1)
        assert field in lib.chm_last_error(), (plan, stage, lib.chm_last_error())

    for stage, rmax in ((2, rmax2), (3, rmax3)):
        refused("f32", stage, rmax, b"d_rmax")
        refused("f32", stage, split, b"d_split")
        refused("split16", stage, split, b"d_split")
        refused("split16_ps", stage, rmax, b"d_rmax")
    b = batches("a", name, P, "f32")
    run(b, P, 2, ins=ins2, outs=s2, inouts={"flags": torch.zeros(128, dtype=torch.int32)}, expect=-1)
    assert b"d_flags" in lib.chm_last_error()
    run(b, P, 2, ins=ins2, outs=dict(s2, Hres=(R * H - H, f32)), expect=-1)
    assert b"n_Hres" in lib.chm_last_error()
    run(b, 3, 2, ins=ins2, outs=s2, expect=-1)
    assert b"pairs" in lib.chm_last_error()
    run(b, P, 3, 2, ins=ins3, outs=s3, inouts=hres, expect=-1)
    assert b"layer" in lib.chm_last_error()
    c = batches("c", name, P, "f32")
    run(c, P, 1, ins={"temb": d["temb"]}, outs={"cin": (P * B * TD, f32)}, tstride=TD, expect=-3)
    assert b"FilmLayer" in lib.chm_last_error()


# ------------------------------------------------------------------------------------------ pairs below max_pairs
@pytest.mark.parametrize("plan", ["split16", "split16_ps"])
def test_one_conditioning_on_a_batch_of_two(world, batches, plan):
    """pairs = 1 on a batch created for two conditionings (a plain decoder call on the sampler's batch): the batch's
    row-max rows are then max_pairs N apart while the call covers N rows. Same bits as on a batch of one."""
    name = "odd"
    d = world["in"]["a", name, 1]
    B, N = len(d["natoms"]), sum(d["natoms"])
    f32 = torch.float32
    extra2 = {"rmax": (N, f32)} if plan == "split16" else {"split": (N * 2 * H, torch.float16), "exp": (N, torch.int32)}
    extra3 = dict(extra2, rmax=(4 * N, f32)) if plan == "split16" else extra2
    calls = ((2, {"a": d["a"], "lat": d["lat"]}, dict({"Hres": (N * H, f32), "gbias": (2 * B * H, f32)}, **extra2), None),
             (3, {"Y": d["Y"][:1], "cemb": d["cemb"][:1]}, dict({"Hl": (N * H, f32)}, **extra3),
              {"Hres": d["Hres"][:1].contiguous()}),
             (4, {"Hres": d["Hres"][:1], "lat": d["lat"], "HO": d["HO"][:N]},
              {"Hf": (N * H, f32), "LAT": (B * 9, f32), "types": (N * 104, f32), "coords": (N * 3, f32)}, None))
    for stage, ins, outs, inouts in calls:
        one = run(batches("a", name, 1, plan), 1, stage, 1, ins=ins, outs=outs, inouts=inouts)
        two = run(batches("a", name, 2, plan), 1, stage, 1, ins=ins, outs=outs, inouts=inouts)
        for q in one:
            same_bits(two[q], one[q], f"{plan} stage {stage} {q}: pairs 1 of max_pairs 2")


# ------------------------------------------------------------------------------------------ knn batches
def test_knn_batches_are_accepted(world, batches):
    """The node-side stages do not depend on the edges: a knn batch gives the bits an fc batch gives (it has no pair
    grid, so no flag words)."""
    from chemeleon_amd.modules.cspnet import CSPNet
    lib = _lib.load()
    name, P = "123", 1
    d = world["in"]["a", name, P]
    cfg = dict(C.config("a"), edge_style="knn")
    net = CSPNet(hidden_dim=cfg["hidden_dim"], time_dim=cfg["time_dim"], text_dim=cfg["text_dim"],
                 num_layers=cfg["num_layers"], max_atoms=cfg["max_atoms"], act_fn=cfg["act_fn"], dis_emb=cfg["dis_emb"],
                 num_freqs=cfg["num_freqs"], edge_style="knn", cutoff=cfg["cutoff"], max_neighbors=cfg["max_neighbors"],
                 ln=cfg["ln"], ip=cfg["ip"], smooth=cfg["smooth"], pred_atom_types=cfg["pred_atom_types"])
    net.load_state_dict(C.state_dict("a"))
    net = net.to(DEV).eval()
    k = net.hip_batch(C.SHAPES[name], max_pairs=P, private=True)
    assert k.knn and int(lib.chm_debug_node_flag_words(k.handle, P, None)) == 0
    f = batches("a", name, P, "split16")
    B, N = len(d["natoms"]), sum(d["natoms"])
    f32 = torch.float32
    s2 = {"Hres": (N * H, f32), "gbias": (2 * B * H, f32), "rmax": (N, f32)}
    s3 = {"Hl": (N * H, f32), "rmax": (4 * N, f32)}
    s4 = {"Hf": (N * H, f32), "LAT": (B * 9, f32), "types": (N * 104, f32), "coords": (N * 3, f32)}
    for stage, ins, outs, inouts in ((2, {"a": d["a"], "lat": d["lat"]}, s2, None),
                                     (3, {"Y": d["Y"][:P], "cemb": d["cemb"][:P]}, s3, {"Hres": d["Hres"][:P].contiguous()}),
                                     (4, {"Hres": d["Hres"][:P], "lat": d["lat"], "HO": d["HO"][:N]}, s4, None)):
        on_fc = run(f, P, stage, 1, ins=ins, outs=outs, inouts=inouts)
        on_knn = run(k, P, stage, 1, ins=ins, outs=outs, inouts=inouts)
        for q in on_fc:
            same_bits(on_knn[q], on_fc[q], f"knn stage {stage} {q}")


# ------------------------------------------------------------------------------------------ 33 layers end to end
@pytest.mark.parametrize("math", ["split16", "f32"])
def test_model_b_forward_against_the_oracle(world, nets, math):
    """One chm_decoder_forward of the 33-layer model (its per-graph terms come from three launches) against the CPU
    oracle, at the tolerance of test_gpu_parity.close."""
    net = nets("b")
    net.set_option("node_ps", 0)
    net.set_option("edge_layer_min", 256)  # (the schedule a batch of this size takes by default)
    net.set_option("edge_rows_short", 1)
    net.set_math(math)
    d = world["in"]["b", "123", 1]
    nat = torch.tensor(d["natoms"])
    B = len(nat)
    x = torch.rand(int(nat.sum()), 3, generator=torch.Generator().manual_seed(5))
    te = O.time_embedding(torch.full((B,), 321, dtype=torch.long), TD).float()
    # (plain embedding rows: the planted ones are for the stage tests. A big_mean row alone costs the fp32 LayerNorm,
    # the oracle's included, 1e-1 of its output, as the baselines of this file show)
    a = torch.randint(len(C.KINDS), 104, (int(nat.sum()),), generator=torch.Generator().manual_seed(6))
    out = net(a.to(DEV), x.to(DEV), d["lat"].to(DEV), nat.to(DEV), d["n2g"].to(DEV), t=te.to(DEV))
    rt, rl, rc, rh = O.cspnet_forward(C.state_dict("b"), C.config("b"), a, x, d["lat"], nat, d["n2g"], te, None)
    e = [close(out.node_features.cpu(), rh, what="nodes"), close(out.atom_types_out.cpu(), rt, what="types"),
         close(out.coords_out.cpu(), rc, what="coords"), close(out.lattice_out.cpu(), rl, what="lattice")]
    print(f"model (b) {math}: scaled errors nodes {e[0]:.2e}, types {e[1]:.2e}, coords {e[2]:.2e}, lattice {e[3]:.2e}")
    net.set_math("split16")
    net.set_option("edge_layer_min", 1)
    net.set_option("edge_rows_short", 0)


def test_measured_table(world):
    """(prints the table of profiles/r15/node_unit/README.md from this session's runs; asserts the margin once more)"""
    for q in sorted(MEASURED):
        b, v = world["base"][q], MEASURED[q]
        print(f"| {q} | {b:.3e} | {v:.3e} | {v / b if b else 0.0:.2f} |")
    assert all(MEASURED[q] <= MARGIN * world["base"][q] for q in MEASURED)
