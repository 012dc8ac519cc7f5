"""CPU checks of the node-side test harness (tests/node_cases.py) and of chm_debug_node_stage's argument checks.

The float64 reference is pinned to the torch modules of chemeleon_amd/modules/cspnet.py cast to float64 (FilmLayer's
norm, the layers' LayerNorms, the final LayerNorm, the lattice head, and the lattice-inner-product column block of
the first edge-MLP Linear) and to oracle/chemeleon_oracle.py (its LayerNorm, its FiLM lines, its conditioning
input, and cspnet_forward's tail from the hidden state it returns). The float32 restatement stays finite on every
case and returns the LayerNorm bias exactly for a constant row; split_rows (the numpy model of the pre-split rows)
holds its own edge cases."""

import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chemeleon_amd import _lib
from chemeleon_amd.modules.cspnet import CSPNet
from oracle import chemeleon_oracle as O

from . import node_cases as C

H = C.H


def net_of(model):
    cfg = C.config(model)
    net = CSPNet(hidden_dim=cfg["hidden_dim"], time_dim=cfg["time_dim"], text_dim=cfg["text_dim"],
                 num_layers=cfg["num_layers"], max_atoms=cfg["max_atoms"], act_fn=cfg["act_fn"], dis_emb=cfg["dis_emb"],
                 num_freqs=cfg["num_freqs"], edge_style=cfg["edge_style"], cutoff=cfg["cutoff"],
                 max_neighbors=cfg["max_neighbors"], ln=cfg["ln"], ip=cfg["ip"], smooth=cfg["smooth"],
                 pred_atom_types=cfg["pred_atom_types"])
    net.load_state_dict(C.state_dict(model))
    return net


def close64(got, want, what, tol=1e-9):
    """Two float64 forms of one formula. The bound is the big_mean rows' conditioning: a mean of 1e4 taken off a
    spread of 1e-2 leaves 1e6 x 2^-53 ~ 1e-10 of the row's deviations, times a few operations."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert err.max() <= tol, f"{what}: {err.max():.3e}"


# ---------------------------------------------------------------- the float64 reference against cspnet.py's modules
@pytest.mark.parametrize("model", ["a", "c"])
def test_reference_matches_the_modules(model):
    net = net_of(model).double()
    sd = C.state_dict(model)
    film = model == "a"
    for name, P in (("123", 2), ("unroll", 1)):
        d = C.inputs(name, P, model)
        h = d["Hres"][:P].double()
        if film:
            ce = d["cemb"][:P].double()[:, d["n2g"]]
            h = F.silu(net.film_layer.norm(d["Y"][:P].double()) * ce[..., :H] + ce[..., H:]) + h
        hl = net.csp_layer_0.layer_norm(h)
        rh, rl = C.film_ln64(sd, 0, d, P, film)
        close64(rh, h.detach(), f"{model} {name} Hres")
        close64(rl, hl.detach(), f"{model} {name} Hl")
        hf = net.final_layer_norm(d["Hres"][:P].double())
        lat = torch.stack([net.lattice_out(O.scatter_mean(hf[c], d["n2g"], len(d["natoms"]))).view(-1, 3, 3) @ d["lat"].double()
                           for c in range(P)])
        rf, rlat = C.tail64(sd, d, P)
        close64(rf, hf.detach(), f"{model} {name} Hf")
        close64(rlat, lat.detach(), f"{model} {name} LAT")


def test_graph_bias_is_the_ip_block_of_the_first_edge_linear():
    """All 33 layers of model (b): edge_mlp[0] on an input that is zero outside the nine inner products."""
    net, sd = net_of("b"), C.state_dict("b")
    d = C.inputs("123", 1, "b")
    L = C.MODELS["b"]["num_layers"]
    assert L > 2 * C.GB_LAYERS and L % C.GB_LAYERS == 1
    ref = C.graph_bias64(sd, L, d["lat"])
    lat = d["lat"].double()
    ein = torch.zeros(len(d["natoms"]), 2 * H + 9 + 6 * 128, dtype=torch.float64)
    ein[:, 2 * H:2 * H + 9] = (lat @ lat.transpose(-1, -2)).reshape(-1, 9)
    for l in range(L):
        lin = copy.deepcopy(getattr(net, f"csp_layer_{l}").edge_mlp[0]).double()
        close64(ref[l], lin(ein).detach(), f"layer {l}")
    close64(C.graph_bias32(sd, L, d["lat"]), ref, "float32 restatement", tol=1e-5)


# ---------------------------------------------------------------- ... and against the oracle
def test_reference_matches_the_oracle():
    sd = {k: v.double() for k, v in C.state_dict("a").items()}
    d = C.inputs("123", 2, "a")
    nat = torch.tensor(d["natoms"])
    # the conditioning input per atom (cspnet_forward's cond_in) is cin's row of the atom's crystal
    cin = C.cond_in(d, 2, 512)
    for c in range(2):
        want = torch.cat([d["temb"].repeat_interleave(nat, 0), d["text"][c].repeat_interleave(nat, 0)], 1)
        assert torch.equal(cin[c][d["n2g"]], want)
    assert torch.equal(C.cond_in(d, 1, 0), d["temb"][None])
    # FilmLayer.forward's lines and the layer's LayerNorm
    for c in range(2):
        cond = d["cemb"][c].double()[d["n2g"]]
        scale, shift = cond.chunk(2, dim=1)
        h = F.silu(O._ln(d["Y"][c].double(), sd, "film_layer.norm") * scale + shift) + d["Hres"][c].double()
        rh, rl = C.film_ln64(sd, 1, d, 2, True)
        close64(rh[c], h, "Hres")
        close64(rl[c], O._ln(h, sd, "csp_layer_1.layer_norm"), "Hl")
    # the tail, from the hidden state cspnet_forward itself returns (film-less, one layer)
    cfg = C.config("c")
    sdc = {k: v.double() for k, v in C.state_dict("c").items()}
    g = torch.Generator().manual_seed(3)
    hidden = []
    _t, lat, _c, hf = O.cspnet_forward(sdc, cfg, d["a"], torch.rand(6, 3, generator=g).double(), d["lat"].double(), nat,
                                       d["n2g"], hidden=hidden)
    rf, rlat = C.tail64(C.state_dict("c"), dict(d, Hres=hidden[-1][None]), 1)
    close64(rf[0], hf, "Hf")
    close64(rlat[0], lat, "LAT")
    ty, co = C.split_heads(d, 2, 104)
    assert torch.equal(ty.reshape(-1, 104), d["HO"][:, :104]) and torch.equal(co.reshape(-1, 3), d["HO"][:, 104:107])


# ---------------------------------------------------------------- the float32 restatement
@pytest.mark.parametrize("model", ["a", "c"])
def test_float32_restatement_is_finite_and_exact_on_constant_rows(model):
    sd = C.state_dict(model)
    film = model == "a"
    lb, flb = sd["csp_layer_0.layer_norm.bias"].numpy(), sd["final_layer_norm.bias"].numpy()
    seen = 0
    for name, P in C.cases():
        d = C.inputs(name, P, model)
        h, hl = C.film_ln32(sd, 0, d, P, film)
        hf, lat = C.tail32(sd, d, P)
        gb = C.graph_bias32(sd, C.MODELS[model]["num_layers"], d["lat"])
        assert all(np.isfinite(v).all() for v in (h, hl, hf, lat, gb)), (name, P)
        r64 = C.film_ln64(sd, 0, d, P, film) + C.tail64(sd, d, P)
        assert all(bool(torch.isfinite(v).all()) for v in r64)
        const = C.kind_mask(name, P, "const")
        seen += int(const.sum())
        assert (hf[const] == flb).all(), f"{name} P {P}: the final LayerNorm of a constant row is not its bias"
        if not film:
            assert (hl[const] == lb).all(), f"{name} P {P}: the LayerNorm of a constant row is not its bias"
        else:  # (FiLM: Y's constant row leaves LN_f as its bias; the residual row is not constant afterwards)
            fb = sd["film_layer.norm.bias"].numpy()
            y = C._ln32(d["Y"][:P].numpy(), sd["film_layer.norm.weight"].numpy(), fb)
            assert (y[const] == fb).all()
    assert seen >= 8


def test_every_kind_is_planted_and_read():
    sd = C.state_dict("a")
    emb = sd["node_embedding.weight"]
    for k, kind in enumerate(C.KINDS):
        ch = emb[k].abs().reshape(4, 128).max(-1).values
        if kind == "zero":
            assert float(ch.max()) == 0.0
        if kind == "zero_chunk":
            assert [float(v) == 0.0 for v in ch] == [False, False, True, False]
        if kind == "scales":
            assert np.allclose(ch.numpy(), C.CHUNK_MAXIMA, rtol=1e-6, atol=0)
        if kind == "const":
            assert bool((emb[k] == C.CONST).all())
        if kind == "big_mean":
            assert abs(float(emb[k].mean()) - 1e4) < 1 and 1e-3 < float(emb[k].double().std()) < 3e-2
        if kind == "pow2":
            assert [float(v) for v in ch] == [2.0 ** p for p in C.POW2_MAXIMA]
            assert bool((torch.frexp(emb[k])[0].abs() == 0.5).all())
    kinds = set()
    for name, P in C.cases():
        a = C.inputs(name, P, "a")["a"]
        assert int(a.min()) >= 0 and int(a.max()) < 104
        kinds |= {C.KINDS[int(v)] for v in a[:6] if int(v) < 6}
        assert not C.kind_mask(name, 2, "big_mean")[1].any()
    assert kinds == set(C.KINDS)
    assert sum(C.SHAPES["odd"]) % 4 and sum(C.SHAPES["odd"]) % 2
    # up to the largest crystal a fully connected batch takes, alone and in a ragged batch
    assert max(max(s) for s in C.SHAPES.values()) == 256 and C.SHAPES["256"] == [256]
    assert C.SHAPES["big_ragged"] == [1, 255, 2] and max(sum(s) for s in C.SHAPES.values()) == 258
    assert list(C.SHAPES)[:5] == ["1", "123", "unroll", "odd", "80"]  # (a case's planted kinds rotate by its position)


def test_split_rows_model():
    """hi + lo carries the scaled row to 2^-22 of its chunk; exponents: k + 1 for a chunk max of 2^k, 0 for an
    all-zero chunk, negative ones as int8; the layout is [H/16][hi 16 | lo 16]."""
    emb = C.state_dict("a")["node_embedding.weight"][:6].numpy()
    raw, words = C.split_rows(emb)
    e = words.view(np.uint32)[:, None] >> (8 * np.arange(4))[None] & 255
    e = e.astype(np.int8).astype(np.int32)
    assert e[0].tolist() == [0, 0, 0, 0] and e[1][2] == 0
    assert e[2].tolist() == [-99, -9, 1, 16]
    assert e[5].tolist() == [p + 1 for p in C.POW2_MAXIMA]
    r = raw.reshape(6, H // 16, 2, 16).astype(np.float64)
    back = np.ldexp((r[:, :, 0] + r[:, :, 1]).reshape(6, 4, 128), e[:, :, None]).reshape(6, H)
    assert (np.abs(back - emb) <= np.ldexp(1.0, np.repeat(e, 128, 1) - 22)).all()
    assert (raw.reshape(6, H // 16, 2, 16)[3] == np.float16(C.CONST * 0.5 ** 0)).reshape(-1)[:16].all()
    assert np.isfinite(raw.astype(np.float32)).all()


# ---------------------------------------------------------------- chm_debug_node_stage refuses bad arguments (no device)
X = ctypes.c_void_p(0x10000)  # (never dereferenced: every call below is refused before any HIP call)


def call(stage, pairs=1, layer=0, io=True, **fields):
    lib = _lib.load()
    v = _lib.chm_debug_node_io()
    for k in ("temb", "cin", "a", "lat", "Hres", "gbias", "Hl", "HO", "Hf", "LAT"):
        setattr(v, "d_" + k, X)
    for k, val in fields.items():
        setattr(v, k, val)
    return lib.chm_debug_node_stage(None, pairs, stage, layer, ctypes.byref(v) if io else None, None)


@pytest.mark.parametrize("kw,field", [
    (dict(stage=1, io=False), b"io"), (dict(stage=0), b"stage"), (dict(stage=5), b"stage"),
    (dict(stage=2, pairs=0), b"pairs"), (dict(stage=3, layer=-1), b"layer"),
    (dict(stage=1, d_temb=None), b"d_temb"), (dict(stage=1, d_cin=None), b"d_cin"),
    (dict(stage=1, tstride=-1), b"tstride"),
    (dict(stage=2, d_a=None), b"d_a"), (dict(stage=2, d_lat=None), b"d_lat"), (dict(stage=2, d_Hres=None), b"d_Hres"),
    (dict(stage=2, d_gbias=None), b"d_gbias"), (dict(stage=2, d_split=X), b"d_exp"), (dict(stage=2, d_exp=X), b"d_split"),
    (dict(stage=3, d_Hres=None), b"d_Hres"), (dict(stage=3, d_Hl=None), b"d_Hl"), (dict(stage=3, d_exp=X), b"d_split"),
    (dict(stage=4, d_Hres=None), b"d_Hres"), (dict(stage=4, d_lat=None), b"d_lat"), (dict(stage=4, d_HO=None), b"d_HO"),
    (dict(stage=4, d_Hf=None), b"d_Hf"), (dict(stage=4, d_LAT=None), b"d_LAT"),
    (dict(stage=1), b"batch"), (dict(stage=2), b"batch"), (dict(stage=3), b"batch"), (dict(stage=4), b"batch"),
])
def test_hook_refuses_bad_arguments_without_a_device(kw, field):
    lib = _lib.load()
    assert call(**kw) == -1, kw
    err = lib.chm_last_error()
    assert b"chm_debug_node_stage" in err and field in err, (kw, err)


def test_flag_words_needs_a_batch():
    lib = _lib.load()
    assert lib.chm_debug_node_flag_words(None, 1, None) == -1 and b"batch" in lib.chm_last_error()
