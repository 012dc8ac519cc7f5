"""CPU reference of the decoder's node-side kernels (k_cond_in, k_embed with its folded per-graph terms, k_graph_bias,
k_film_ln, k_layer_norm, k_graph_heads, k_split_heads and the store_split_row512 helper; csrc/kernels.hip) and the
inputs their tests share. Test infrastructure only.

The four stages are those of chm_debug_node_stage (include/chemeleon_hip.h). Each has two forms on the same inputs:
  float64: the operation itself, widened (the fp32 weights and inputs included). tests/test_node_cases.py pins it to
    the torch modules of chemeleon_amd/modules/cspnet.py cast to float64, and to oracle/chemeleon_oracle.py where
    the oracle has the piece.
  float32: a restatement in the kernel's order with every operation rounded to fp32 (numpy): the two-pass LayerNorm
    with eps 1e-5 and the biased variance, SiLU as x / (1 + exp(-x)), the node sums of the lattice head in node
    order, the per-graph term as bias + the nine products in (i, j) order. It is the yardstick of the device's
    error, not a bit-exact model of it (the device sums a row across a wave and fuses products into FMAs).

Rows that kernels get wrong are planted by name (KINDS): in the embedding table (stage 2 reads them through the
atom types) and in the rows of Hres / Y (stages 3 and 4)."""

import functools
import zlib

import numpy as np
import torch

from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict

H, TD, HEADS_N, GB_LAYERS = 512, 128, 128, 16
EPS = 1e-5
# (256 / big_ragged: the largest crystal a fully connected batch takes, alone and between small ones: the loops and
# reductions over a crystal's atoms at three times the reference workload's 80)
SHAPES = {"1": [1], "123": [1, 2, 3], "unroll": [7, 8, 9, 16, 17], "odd": [5] * 3, "80": [80],
          "256": [256], "big_ragged": [1, 255, 2]}
PAIRS = (1, 2)
# (a) FiLM, (b) time only with 33 layers (per-graph terms in groups of 16 + 16 + 1), (c) no FilmLayer,
# (d) = (a) with 1 and 125 atom classes (the tail only: 125 + 3 fills the packed head rows)
MODELS = {"a": dict(text_dim=512, time_dim=128, num_layers=2, max_atoms=104),
          "b": dict(text_dim=0, time_dim=128, num_layers=33, max_atoms=104),
          "c": dict(text_dim=0, time_dim=0, num_layers=1, max_atoms=104),
          "d1": dict(text_dim=512, time_dim=128, num_layers=2, max_atoms=1),
          "d125": dict(text_dim=512, time_dim=128, num_layers=2, max_atoms=125)}
# the planted rows; KINDS[k] is row k of the embedding table of the models with >= 6 classes
KINDS = ("zero", "zero_chunk", "scales", "const", "big_mean", "pow2")
CONST = 0.75  # (k * 0.75 is exact in fp32 for every k <= 512: a constant row's mean is exact in any summation order)
CHUNK_MAXIMA = (1e-30, 1e-3, 1.0, 6e4)
POW2_MAXIMA = (0, -14, 15, -3)  # chunk maxima 2^k: frexp(2^k) = (0.5, k + 1), the edge of the exponent rule


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def planted_row(kind, g):
    """One 512-wide fp32 row of the named kind."""
    r = torch.randn(H, generator=g)
    if kind == "zero":
        return torch.zeros(H)
    if kind == "zero_chunk":
        r[256:384] = 0.0
        return r
    if kind == "scales":
        for c, top in enumerate(CHUNK_MAXIMA):
            ch = r[128 * c:128 * (c + 1)]
            r[128 * c:128 * (c + 1)] = (ch.double() / ch.abs().max().double() * top).float()
        return r
    if kind == "const":
        return torch.full((H,), CONST)
    if kind == "big_mean":
        return (1e4 + 1e-2 * r.double()).float()
    if kind == "pow2":
        sign = torch.where(r < 0, -1.0, 1.0)
        down = torch.randint(0, 11, (H,), generator=g)
        for c, k in enumerate(POW2_MAXIMA):
            down[128 * c + int(torch.randint(0, 128, (1,), generator=g))] = 0
        k = torch.tensor(POW2_MAXIMA).repeat_interleave(128) - down
        return sign * torch.ldexp(torch.ones(H), k)
    return r  # "plain"


def config(model):
    return dict(default_config(), **MODELS[model])


@functools.lru_cache(maxsize=None)
def state_dict(model):
    """synthetic_state_dict of the model, rows 0..5 of the embedding table replaced by the planted kinds."""
    cfg = config(model)
    sd = synthetic_state_dict(cfg)
    if cfg["max_atoms"] >= len(KINDS):
        for k, kind in enumerate(KINDS):
            sd["node_embedding.weight"][k] = planted_row(kind, _gen("emb", kind))
    return sd


def cases():
    return [(name, P) for name in SHAPES for P in PAIRS]


def row_kinds(name, c):
    """The kind of every node's row for conditioning c: the first nodes take the planted kinds, rotated by the
    case so that a one-node case differs from the next; conditioning 1 gets a plain row in big_mean's place (the
    lattice head of its crystals stays measurable at fp32 level)."""
    N = sum(SHAPES[name])
    rot = list(SHAPES).index(name)
    kinds = ["plain"] * N
    for i in range(min(N, len(KINDS))):
        k = KINDS[(i + rot) % len(KINDS)]
        kinds[i] = "plain" if (c == 1 and k == "big_mean") else k
    return kinds


def planted_rows(name, P, what, scale=1.0):
    rows = torch.empty(P, sum(SHAPES[name]), H)
    for c in range(P):
        for i, kind in enumerate(row_kinds(name, c)):
            r = planted_row(kind, _gen(what, name, c, i))
            rows[c, i] = r * scale if kind == "plain" else r
    return rows


def inputs(name, P, model):
    """Every stage's inputs of one case, fp32 / int64 torch tensors on the CPU."""
    cfg = config(model)
    nat = SHAPES[name]
    B, N, A, X = len(nat), sum(nat), cfg["max_atoms"], cfg["text_dim"]
    g = _gen("inputs", name, P, model)
    d = {"natoms": nat, "n2g": torch.arange(B).repeat_interleave(torch.tensor(nat))}
    a = torch.randint(0, A, (N,), generator=g)
    if A >= len(KINDS):
        rot = list(SHAPES).index(name)
        for i in range(min(N, len(KINDS))):
            a[i] = (i + rot) % len(KINDS)
    d["a"] = a
    d["lat"] = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.5 * torch.randn(B, 3, 3, generator=g)
    # stage 1: a time table read at row t, the same rows per graph, text rows of both conditionings
    d["table"] = torch.randn(7, TD, generator=g)
    d["t"] = 4
    d["temb"] = d["table"][d["t"]].expand(B, TD).contiguous()
    d["temb_rows"] = torch.randn(B, TD, generator=g)  # (per-graph rows: the training forward's form)
    d["text"] = torch.randn(2, B, X, generator=g)
    # stages 3 and 4
    d["Hres"] = planted_rows(name, P, "Hres", 2.0)
    d["Y"] = planted_rows(name, P, "Y")
    d["cemb"] = 0.5 * torch.randn(P, B, 2 * H, generator=g)
    d["HO"] = torch.randn(P * N, HEADS_N, generator=g)
    return d


# ------------------------------------------------------------------------------------------ float64
def _ln64(x, w, b):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * w.double() + b.double()


def _silu64(x):
    return x / (1.0 + torch.exp(-x))


def cond_in(d, P, X, tstride_rows=False):
    """stage 1 (a copy): [time row | text row of conditioning c] per (c, graph)."""
    te = d["temb_rows"] if tstride_rows else d["temb"]
    B = te.shape[0]
    return torch.stack([torch.cat([te, d["text"][c][:, :X]], 1) if X else te.clone() for c in range(P)]).reshape(P, B, TD + X)


def graph_bias64(sd, L, lat):
    """stage 2: out[l][g] = b1_l + W1_l[:, 2H:2H+9] vec(L_g L_g^T)."""
    llt = (lat.double() @ lat.double().transpose(-1, -2)).reshape(-1, 9)
    return torch.stack([sd[f"csp_layer_{l}.edge_mlp.0.bias"].double() +
                        llt @ sd[f"csp_layer_{l}.edge_mlp.0.weight"][:, 2 * H:2 * H + 9].double().T for l in range(L)])


def film_ln64(sd, layer, d, P, film):
    """stage 3: (Hres', Hl). FiLM: Hres' = SiLU(LN_f(Y) scale_g + shift_g) + Hres; Hl = LN_l(Hres')."""
    h = d["Hres"][:P].double()
    if film:
        ce = d["cemb"][:P].double()[:, d["n2g"]]  # [P, N, 2H]
        y = _ln64(d["Y"][:P], sd["film_layer.norm.weight"], sd["film_layer.norm.bias"])
        h = _silu64(y * ce[..., :H] + ce[..., H:]) + h
    p = f"csp_layer_{layer}.layer_norm."
    return h, _ln64(h, sd[p + "weight"], sd[p + "bias"])


def tail64(sd, d, P):
    """stage 4: (Hf, LAT): the final LayerNorm; the graph means through lattice_out, times the lattice."""
    hf = _ln64(d["Hres"][:P], sd["final_layer_norm.weight"], sd["final_layer_norm.bias"])
    B = len(d["natoms"])
    gm = torch.zeros(P, B, H, dtype=torch.float64).index_add_(1, d["n2g"], hf)
    gm = gm / torch.tensor(d["natoms"], dtype=torch.float64)[None, :, None]
    l9 = (gm @ sd["lattice_out.weight"].double().T).reshape(P, B, 3, 3)
    return hf, l9 @ d["lat"].double()


def split_heads(d, P, A):
    """stage 4 (copies): types = HO[:, :A], coords = HO[:, A:A+3]."""
    N = sum(d["natoms"])
    ho = d["HO"][:P * N]
    return ho[:, :A].reshape(P, N, A).clone(), ho[:, A:A + 3].reshape(P, N, 3).clone()


# ------------------------------------------------------------------------------------------ float32, kernel order
F32 = np.float32


def _ln32(x, w, b):
    x = np.asarray(x, F32)
    mean = (x.sum(-1, keepdims=True, dtype=F32) * F32(1.0 / H)).astype(F32)
    dd = (x - mean).astype(F32)
    var = ((dd * dd).sum(-1, keepdims=True, dtype=F32) * F32(1.0 / H)).astype(F32)
    rstd = (F32(1.0) / np.sqrt(var + F32(EPS), dtype=F32)).astype(F32)
    return ((dd * rstd).astype(F32) * np.asarray(w, F32) + np.asarray(b, F32)).astype(F32)


def _silu32(x):
    with np.errstate(over="ignore"):
        return (x / (F32(1.0) + np.exp(-x, dtype=F32))).astype(F32)


def graph_bias32(sd, L, lat):
    lat = lat.numpy().astype(F32)
    out = []
    for l in range(L):
        wc = sd[f"csp_layer_{l}.edge_mlp.0.weight"][:, 2 * H:2 * H + 9].numpy()
        v = np.repeat(sd[f"csp_layer_{l}.edge_mlp.0.bias"].numpy()[None], lat.shape[0], 0).astype(F32)
        for i in range(3):
            for j in range(3):
                ip = ((lat[:, i, 0] * lat[:, j, 0] + lat[:, i, 1] * lat[:, j, 1]).astype(F32) + lat[:, i, 2] * lat[:, j, 2]).astype(F32)
                v = (v + wc[None, :, 3 * i + j] * ip[:, None]).astype(F32)
        out.append(v)
    return np.stack(out)


def film_ln32(sd, layer, d, P, film):
    h = d["Hres"][:P].numpy().astype(F32)
    if film:
        ce = d["cemb"][:P].numpy()[:, d["n2g"].numpy()]
        y = _ln32(d["Y"][:P].numpy(), sd["film_layer.norm.weight"].numpy(), sd["film_layer.norm.bias"].numpy())
        h = (_silu32(((y * ce[..., :H]).astype(F32) + ce[..., H:]).astype(F32)) + h).astype(F32)
    p = f"csp_layer_{layer}.layer_norm."
    return h, _ln32(h, sd[p + "weight"].numpy(), sd[p + "bias"].numpy())


def tail32(sd, d, P):
    hf = _ln32(d["Hres"][:P].numpy(), sd["final_layer_norm.weight"].numpy(), sd["final_layer_norm.bias"].numpy())
    nat, lat = d["natoms"], d["lat"].numpy().astype(F32)
    wl = sd["lattice_out.weight"].numpy()
    out = np.zeros((P, len(nat), 3, 3), F32)
    for c in range(P):
        off = 0
        for g, n in enumerate(nat):
            s = np.zeros(H, F32)
            for k in range(n):  # the node sum in node order
                s = (s + hf[c, off + k]).astype(F32)
            off += n
            mean = (s / F32(n)).astype(F32)
            l9 = (wl * mean[None]).astype(F32).sum(-1, dtype=F32).reshape(3, 3)
            for a in range(3):
                for b in range(3):
                    out[c, g, a, b] = F32(F32(l9[a, 0] * lat[g, 0, b] + l9[a, 1] * lat[g, 1, b]) + l9[a, 2] * lat[g, 2, b])
    return hf, out


# ------------------------------------------------------------------------------------------ the derived outputs
def split_rows(x):
    """What store_split_row512 writes for fp32 rows x [R, 512] (numpy): (raw fp16 [R, 2H] in the
    [H/16][hi 16 | lo 16] layout, packed exponent words int32 [R]). e = frexp exponent of each 128-column chunk's
    max |value| (0 for an all-zero chunk); hi = fp16(x 2^-e), lo = fp16(x 2^-e - hi), round to nearest even."""
    x = np.asarray(x, F32)
    R = x.shape[0]
    m = np.abs(x).reshape(R, 4, 128).max(-1)
    e = np.where(m > 0, np.frexp(m)[1], 0).astype(np.int32)
    xs = np.ldexp(x.reshape(R, 4, 128), -e[:, :, None]).astype(F32).reshape(R, H)  # (a power-of-two scale: exact)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(F32)).astype(F32).astype(np.float16)
    raw = np.stack([hi.reshape(R, H // 16, 16), lo.reshape(R, H // 16, 16)], 2).reshape(R, 2 * H)
    words = ((e[:, 0] & 255) | ((e[:, 1] & 255) << 8) | ((e[:, 2] & 255) << 16) | ((e[:, 3] & 255) << 24))
    return raw, words.astype(np.uint32).view(np.int32)


def row_max(x):
    return np.abs(np.asarray(x, F32)).reshape(-1, H).max(-1)


def kind_mask(name, P, kind):
    """[P, N] bool: rows of the named kind."""
    return np.array([[k == kind for k in row_kinds(name, c)] for c in range(P)])


def graph_mask(name, P, kind):
    """[P, B] bool: crystals holding a row of the named kind."""
    nat = SHAPES[name]
    n2g = np.repeat(np.arange(len(nat)), nat)
    km = kind_mask(name, P, kind)
    return np.array([[bool(km[c][n2g == g].any()) for g in range(len(nat))] for c in range(P)])
