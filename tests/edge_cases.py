"""Operands, the float64 reference and the error metric of the per-layer message-path tests
(tests/test_edge_cases.py on the CPU, tests/test_gpu_edge_layer.py on the GPU), the counterpart of
tests/gemm_cases.py. A plain helper module: every operand is seeded.

One CSP layer's message path on fc edges (include/chemeleon_hip.h, chm_debug_edge_layer):
    agg[c][i] = mean_j SiLU(SiLU(D f_ij + P_c[i] + Q_c[j]) W2^T + b2),
f_ij = [sin(arg) | cos(arg)] the Fourier features of edge (i, j), axis-major within each half, P_c / Q_c the
per-node halves of edge layer 1 for conditioning c (P holding b1 and the per-graph term).

The arguments are part of the operation's definition and are computed in float32 exactly as k_fourier rounds
them: d = rem1(fl32(x_j - x_i)), f_k = fl32(fl32(2 pi) k), arg = fl32(d f_k). On the schedules that run edge
layer 1 on unordered pairs (option edge_pairs, split16's default) the kernel defines the reverse edge by the
forward one: for i > j, arg_ij = -arg_ji (sin negated, cos kept; k_edge16_pairs). `pairs=True` takes that
definition; the two differ by up to 8e-5 in a feature, far above fp32 rounding, so each schedule is measured
against its own definition."""

import functools

import numpy as np

H, NF = 512, 128
FD = 6 * NF
U = 2.0 ** -24            # fp32 unit roundoff
GATE_FACTOR = 16.0        # a row's e may be this many times the float32 chain's worst row (floored at U)
DEAD = 1e-30              # rows whose reference maximum is below this must come out below it
FAMILIES = ("normal", "rowscale", "chunkdead", "large")
LAST = float(np.float32(1.0) - np.float32(2.0 ** -24))  # the largest fp32 below 1

# natoms lists of the GPU tests (the largest: 6400 edge rows)
SHAPES = {
    "1": [1], "16": [16], "17": [17], "14": [14], "61": [61], "62": [62], "80": [80],
    "mixed7": [5, 9, 3, 12, 7, 1, 20],
    "tiny55": [1] * 40 + [2] * 10 + [3] * 5,
    "ragged5": [23, 7, 40, 1, 80],
}
# crystals of 81 to 256 atoms, the rest of the range a fully connected batch accepts (the largest: 71 439 edge rows).
# A table of its own: the parametrisations over SHAPES do not multiply. 81: the first size above SHAPES; 127 / 128:
# 64 / 65 pair tiles below the last row tile, one / two passes of the pair grid's flag polling; 193+: above 192 atoms
# (no 192-row tiles) in a ragged batch; 255: every node cut by a tile edge at another offset; 256: a node's rows are
# one row tile; ragged256: the batch of tests/test_row_tiles.py.
BIG_SHAPES = {
    "81": [81], "127": [127], "128": [128], "193+": [193, 20, 20], "255": [255], "256": [256],
    "ragged256": [1, 255, 2, 80, 3],
}
ALL_SHAPES = {**SHAPES, **BIG_SHAPES}
# edge rows per block of source nodes in ref64 / base32: every shape of SHAPES is one block, as it always was; a big
# shape's feature matrix (65 536 x 768) is never allocated whole
REF_BLOCK_ROWS = 16384


def node_blocks(natoms, max_rows=None):
    """[(first node, end node, first edge row, end edge row)]: consecutive source nodes whose edge rows (a node's
    rows are contiguous) number at most max_rows (REF_BLOCK_ROWS), one node at the least."""
    max_rows = REF_BLOCK_ROWS if max_rows is None else max_rows
    n = node_counts(natoms)
    end = np.cumsum(n)
    out, a = [], 0
    while a < len(n):
        r0 = int(end[a] - n[a])
        b = max(a + 1, int(np.searchsorted(end, r0 + max_rows, side="right")))
        out.append((a, b, r0, int(end[b - 1])))
        a = b
    return out


def fc_edges(natoms):
    """(ei, ej) of the fc edges in the decoder's row order (oracle fc_edges): per crystal row-major (i, j), self
    edges included."""
    ei, ej, off = [], [], 0
    for n in natoms:
        a = np.arange(n) + off
        ei.append(np.repeat(a, n))
        ej.append(np.tile(a, n))
        off += n
    return np.concatenate(ei), np.concatenate(ej)


def node_counts(natoms):
    """n of each node's crystal [N]: the node's edge count."""
    return np.repeat(np.asarray(natoms), np.asarray(natoms))


def frac_coords(natoms, kind="uniform", seed=0):
    """[N, 3] float32. 'edge': coordinates at 0 and at 1 - 2^-24 and coincident atoms, so d = 0 and d just below 1
    occur (rows cycle: all 0 / all 1 - 2^-24 / a copy of the row before / random with one coordinate at 0)."""
    N = int(sum(natoms))
    rng = np.random.default_rng([seed, N, len(natoms), kind == "edge"])
    x = rng.random((N, 3), dtype=np.float32)
    if kind == "edge":
        for r in range(N):
            if r % 4 == 0:
                x[r] = 0.0
            elif r % 4 == 1:
                x[r] = LAST
            elif r % 4 == 2:
                x[r] = x[r - 1] if r % 8 == 2 else x[r - 2]
            else:
                x[r, r % 3] = 0.0
    return x


def rem1(x):
    """torch.remainder(x, 1.0) in fp32 as k_fourier's rem1: fmod, negatives shifted by +1 (fp32 addition)."""
    m = np.fmod(np.asarray(x, np.float32), np.float32(1.0))
    return np.where(m < 0, (m + np.float32(1.0)).astype(np.float32), m).astype(np.float32)


def fourier_args(frac, ei, ej, pairs=False):
    """arg [E, 3 NF] float32, axis-major, every operation a correctly rounded fp32 one."""
    frac = np.asarray(frac, np.float32)
    f = (np.float32(2.0 * np.pi) * np.arange(NF, dtype=np.float32)).astype(np.float32)
    if pairs:
        lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
        d = rem1(frac[hi] - frac[lo])
    else:
        d = rem1(frac[ej] - frac[ei])
    arg = (d[:, :, None] * f[None, None, :]).astype(np.float32).reshape(len(ei), 3 * NF)
    if pairs:
        arg = np.where((ei > ej)[:, None], -arg, arg)
    return arg


def layer_weights(sd, layer):
    """float32 numpy weights of CSP layer `layer` from a state dict, sliced as chm_model_create slices
    edge_mlp.0.weight [H][2H + 9 + FD]: WA = [:, 0:H] (h_i), WB = [:, H:2H] (h_j), C = [:, 2H:2H+9] (lattice inner
    products), D = [:, 2H+9:] (Fourier features)."""
    p = f"csp_layer_{layer}."
    g = lambda k: np.ascontiguousarray(sd[p + k].detach().cpu().float().numpy())  # noqa: E731
    W1 = g("edge_mlp.0.weight")
    assert W1.shape == (H, 2 * H + 9 + FD)
    return dict(WA=W1[:, :H], WB=W1[:, H:2 * H], C=W1[:, 2 * H:2 * H + 9], D=np.ascontiguousarray(W1[:, 2 * H + 9:]),
                b1=g("edge_mlp.0.bias"), W2=g("edge_mlp.2.weight"), b2=g("edge_mlp.2.bias"))


def silu64(x):
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def ref64(natoms, frac, PQ, w, pairs=False):
    """agg [P, N, H] float64: float64 from the fp32 arguments on. PQ [P, N, 2H] float32, w = layer_weights().
    Computed per block of source nodes (node_blocks)."""
    ei, ej = fc_edges(natoms)
    Dt = w["D"].astype(np.float64).T
    PQ = np.asarray(PQ, np.float64)
    W2t, b2 = w["W2"].astype(np.float64).T, w["b2"].astype(np.float64)
    n = node_counts(natoms)
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    out = np.empty((PQ.shape[0], len(n), H))
    for a, b, r0, r1 in node_blocks(natoms):
        bi, bj = ei[r0:r1], ej[r0:r1]
        arg = fourier_args(frac, bi, bj, pairs).astype(np.float64)
        DF = np.concatenate([np.sin(arg), np.cos(arg)], 1) @ Dt
        for c in range(PQ.shape[0]):
            S = silu64(DF + PQ[c, bi, :H] + PQ[c, bj, H:])
            M = silu64(S @ W2t + b2)
            out[c, a:b] = np.add.reduceat(M, starts[a:b] - r0, axis=0) / n[a:b, None]
    return out


def base32(natoms, frac, PQ, w, pairs=False):
    """The same chain in torch float32 on the CPU (the baseline, as baseline_eta is for the GEMMs): sin / cos of the
    same fp32 arguments, F.linear, F.silu, scatter-add mean, per block of source nodes. [P, N, H] float32 numpy."""
    import torch
    import torch.nn.functional as F
    ei, ej = fc_edges(natoms)
    Dt = torch.from_numpy(w["D"]).T
    PQ = torch.tensor(np.asarray(PQ, np.float32))
    W2, b2 = torch.from_numpy(w["W2"]), torch.from_numpy(w["b2"])
    n = torch.from_numpy(node_counts(natoms)).float()
    out = torch.empty(PQ.shape[0], len(n), H)
    for a, b, r0, r1 in node_blocks(natoms):
        arg = torch.from_numpy(fourier_args(frac, ei[r0:r1], ej[r0:r1], pairs))
        DF = torch.cat([arg.sin(), arg.cos()], 1) @ Dt
        ti, tj = torch.from_numpy(ei[r0:r1]), torch.from_numpy(ej[r0:r1])
        for c in range(PQ.shape[0]):
            S = F.silu(DF + PQ[c, ti, :H] + PQ[c, tj, H:])
            M = F.silu(F.linear(S, W2, b2))
            out[c, a:b] = torch.zeros(b - a, H).index_add_(0, ti - a, M) / n[a:b, None]
    return out.numpy()


def row_errors(agg, ref):
    """(e [P, N], dead_ok): per output row e = max_k |agg - ref| / max_k |ref|; rows whose reference maximum is
    below DEAD count e = 0 and must have |agg| <= DEAD (dead_ok). Non-finite agg rows give e = inf."""
    agg, ref = np.asarray(agg, np.float64), np.asarray(ref, np.float64)
    den = np.abs(ref).max(-1)
    live = den >= DEAD
    with np.errstate(invalid="ignore"):
        e = np.where(live, np.abs(agg - ref).max(-1) / np.where(live, den, 1.0), 0.0)
    e = np.where(np.isfinite(agg).all(-1), e, np.inf)
    dead_ok = bool((live | (np.abs(agg).max(-1) <= DEAD)).all())
    return e, dead_ok


def max_row_error(agg, ref):
    e, dead_ok = row_errors(agg, ref)
    return (float(e.max()) if dead_ok else float("inf"))


def gate(base_e):
    return GATE_FACTOR * max(base_e, U)


DEAD_P, LARGE_P = -200.0, 40.0


def dead_nodes(N):
    """chunkdead: the nodes whose four chunks are all dead."""
    return np.arange(N) % 7 == 3


@functools.lru_cache(maxsize=None)
def pq(family, N, P=2, seed=0):
    """[P, N, 2H] float32, read-only. Rows do not depend on P: pq(f, N, 1) is pq(f, N, 2)[:1].
    normal: N(0, 1). rowscale: node rows scaled by 2^+6 or 2^-6, so neighbouring S rows carry different chunk
    exponents. chunkdead: P = -200 on the 128-column chunk (node % 4) of every node, so that chunk of S is exactly
    +-0 in fp32 (SiLU(-200 + O(10)): exp overflows), and on all four chunks of the nodes dead_nodes(N). large: P + 40
    on chunk (node % 4): S ~ z there, big exponents next to small ones."""
    if P != 2:
        return pq(family, N, 2, seed)[:P]
    rng = np.random.default_rng([seed, N, FAMILIES.index(family)])
    x = rng.standard_normal((2, N, 2 * H)).astype(np.float32)
    if family == "rowscale":
        x = x * (2.0 ** (6 * (2 * rng.integers(0, 2, (1, N, 1)) - 1))).astype(np.float32)
    elif family in ("chunkdead", "large"):
        for i in range(N):
            c = i % 4
            if family == "large":
                x[:, i, 128 * c:128 * c + 128] += np.float32(LARGE_P)
            else:
                x[:, i, 128 * c:128 * c + 128] = DEAD_P
                if dead_nodes(N)[i]:
                    x[:, i, :H] = DEAD_P
    x.setflags(write=False)
    return x


def split_rows_value(split, exps):
    """(hi + lo) 2^e of the pre-split node GEMMs' rows (store_split_row512's layout): split [R][H/16][2][16] fp16
    (hi 16 | lo 16 per 16-column group), exps [R] the packed int8 exponents of the four 128-column chunks.
    Returns (value [R, H] float64, hi, lo, e [R, 4])."""
    s = np.asarray(split).view(np.float16).reshape(-1, H // 16, 2, 16).astype(np.float64)
    hi, lo = s[:, :, 0, :].reshape(-1, H), s[:, :, 1, :].reshape(-1, H)
    e = np.asarray(exps, np.int32).view(np.int8).reshape(-1, 4).astype(np.int64)
    return (hi + lo) * np.repeat(2.0 ** e, 128, axis=1), hi, lo, e
