"""CPU checks of the message-path test harness (tests/edge_cases.py) and of chm_debug_edge_layer's argument checks.

The float64 reference of tests/test_gpu_edge_layer.py must be the operation the decoder runs: with P and Q computed
from node features, the lattice term and b1 the way the decoder does, it agrees with the oracle's CSPLayer messages
and aggregation (oracle/chemeleon_oracle.py csp_messages) to float32 accuracy, which also proves the slicing of
edge_mlp.0.weight. The operand families stay finite, the gate refuses a 2^-16 error, and the hook refuses bad
arguments with CHM_E_ARG naming the field before any HIP call, so those checks run here without a device."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict
from oracle import chemeleon_oracle as O
from tests import edge_cases as EC

H = EC.H


@functools.lru_cache(maxsize=None)
def _sd():
    return synthetic_state_dict(default_config())


def _decoder_pq(natoms, w, seed):
    """(frac, lattices, hl, PQ [1, N, 2H] float32) with [P | Q] = hl [WA ; WB]^T, P += b1 + C vec(L L^T), in fp32."""
    g = torch.Generator().manual_seed(seed)
    N, B = sum(natoms), len(natoms)
    hl = torch.randn(N, H, generator=g)
    lat = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    llt = (lat @ lat.transpose(-1, -2)).reshape(-1, 9)
    n2g = torch.arange(B).repeat_interleave(torch.tensor(natoms))
    P = hl @ torch.from_numpy(w["WA"]).T + torch.from_numpy(w["b1"]) + llt[n2g] @ torch.from_numpy(w["C"]).T
    Q = hl @ torch.from_numpy(w["WB"]).T
    frac = EC.frac_coords(natoms, "uniform", seed)
    return frac, lat, hl, torch.cat([P, Q], 1)[None].numpy()


@pytest.mark.parametrize("layer", [0, 5])
@pytest.mark.parametrize("natoms", [[5, 9, 3, 12, 7, 1, 20], [23, 7, 1, 30], EC.BIG_SHAPES["81"]],
                         ids=["mixed7", "ragged4", "81"])
def test_reference_is_the_oracles_message_path(natoms, layer):
    sd, w = _sd(), EC.layer_weights(_sd(), layer)
    frac, lat, hl, PQ = _decoder_pq(natoms, w, 7 + layer)
    edges = O.fc_edges(natoms)
    x = torch.from_numpy(frac)
    fd = (x[edges[1]] - x[edges[0]]) % 1.0
    B = len(natoms)
    e2g = torch.arange(B).repeat_interleave(torch.tensor(natoms))[edges[0]]
    llt = (lat @ lat.transpose(-1, -2)).reshape(-1, 9)
    want = O.csp_messages(sd, f"csp_layer_{layer}.", hl, edges, llt[e2g], O.fourier(fd, EC.NF)).numpy()
    ref = EC.ref64(natoms, frac, PQ, w)[0]
    b32 = EC.base32(natoms, frac, PQ, w)[0]
    e_or, e_b = EC.max_row_error(want, ref), EC.max_row_error(b32, ref)
    print(f"layer {layer} N={sum(natoms)}: oracle vs ref64 {e_or:.3e}, base32 vs ref64 {e_b:.3e}")
    # float32 accuracy: the oracle sums K = 1801 in another order and P / Q were rounded to fp32 on the way
    assert e_or <= 64 * EC.U and e_b <= 64 * EC.U
    # a wrong slice (D taken one column off) is far outside
    w_bad = dict(w, D=np.ascontiguousarray(np.roll(w["D"], 1, axis=1)))
    assert EC.max_row_error(want, EC.ref64(natoms, frac, PQ, w_bad)[0]) > 1e-3


def test_fc_edges_and_rem1_match_torch():
    for nat in ([1], [3, 1, 4], EC.SHAPES["ragged5"], *EC.BIG_SHAPES.values()):
        ei, ej = EC.fc_edges(nat)
        e = O.fc_edges(nat).numpy()
        assert np.array_equal(ei, e[0]) and np.array_equal(ej, e[1])
        assert EC.node_counts(nat).sum() == len(ei)
    x = np.concatenate([np.random.default_rng(0).uniform(-1, 1, 4000), [0.0, -0.0, EC.LAST, -EC.LAST, -2.0 ** -30, 1.0,
                                                                         -1.0]]).astype(np.float32)
    assert np.array_equal(EC.rem1(x), torch.remainder(torch.from_numpy(x), 1.0).numpy())


def test_edge_coordinates_reach_d_zero_and_d_below_one():
    nat = [5, 9, 3]
    x = EC.frac_coords(nat, "edge")
    ei, ej = EC.fc_edges(nat)
    d = EC.rem1(x[ej] - x[ei])
    off = ei != ej
    assert (d[off] == 0).all(1).any(), "no coincident atoms"
    assert (d == np.float32(EC.LAST)).any() and (d == np.float32(2.0 ** -24)).any()
    assert (d >= 0).all() and (d < 1).all()
    arg = EC.fourier_args(x, ei, ej)
    assert arg.dtype == np.float32 and arg.shape == (len(ei), 3 * EC.NF)
    # fl32(2 pi) k d in fp32, one rounding per product
    f = np.float32(6.28318548202514648) * np.float32(127.0)
    assert arg[5, 2 * EC.NF + 127] == np.float32(d[5, 2] * f)


def test_pair_arguments_are_the_forward_edges_negated():
    nat = [4, 7]
    x = EC.frac_coords(nat, "uniform", 3)
    ei, ej = EC.fc_edges(nat)
    a_d, a_p = EC.fourier_args(x, ei, ej), EC.fourier_args(x, ei, ej, pairs=True)
    fwd = ei <= ej
    assert np.array_equal(a_d[fwd], a_p[fwd])
    row = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(ei, ej))}
    for k in np.nonzero(~fwd)[0]:
        assert np.array_equal(a_p[k], -a_d[row[(int(ej[k]), int(ei[k]))]])
    # same features in real arithmetic; in fp32 the two argument roundings differ (edge16.hip: up to 8e-5)
    dsin = np.abs(np.sin(a_d.astype(np.float64)) - np.sin(a_p.astype(np.float64))).max()
    assert 0 < dsin < 2e-4


def test_big_shapes_are_what_they_are_chosen_for():
    """The edge rows of each big shape, the sizes that bracket a threshold, and the tables kept apart."""
    rows = {k: sum(n * n for n in v) for k, v in EC.BIG_SHAPES.items()}
    assert rows == {"81": 6561, "127": 16129, "128": 16384, "193+": 38049, "255": 65025, "256": 65536,
                    "ragged256": 71439}
    assert not set(EC.BIG_SHAPES) & set(EC.SHAPES) and len(EC.ALL_SHAPES) == len(EC.SHAPES) + len(EC.BIG_SHAPES)
    assert max(max(v) for v in EC.SHAPES.values()) == 80 and min(max(v) for v in EC.BIG_SHAPES.values()) == 81
    assert max(max(v) for v in EC.BIG_SHAPES.values()) == 256  # (batch creation refuses 257)
    tiles = lambda n: (n * (n + 1) // 2 + 127) // 128  # noqa: E731
    assert tiles(127) == 64 and tiles(128) == 65  # 64 pair tiles of 128 pairs, then a 65th
    assert max(EC.BIG_SHAPES["193+"]) == 193 and EC.BIG_SHAPES["ragged256"] == [1, 255, 2, 80, 3]
    # the edge coordinates' special rows reach the big shapes too
    x = EC.frac_coords(EC.BIG_SHAPES["128"], "edge")
    assert (x[0] == 0).all() and (x[125] == np.float32(EC.LAST)).all() and (x[126] == x[124]).all()


def test_reference_blocks_tile_the_nodes_and_do_not_change_the_reference(monkeypatch):
    """ref64 / base32 run per block of source nodes: the blocks tile nodes and edge rows in order, hold at most
    REF_BLOCK_ROWS rows, every shape of SHAPES is a single block (its reference is computed as it always was), and
    a reference cut into many blocks equals the one-block reference to float64 rounding."""
    for nat in EC.ALL_SHAPES.values():
        blocks = EC.node_blocks(nat)
        n = EC.node_counts(nat)
        assert blocks[0][0] == 0 and blocks[0][2] == 0 and blocks[-1][1] == len(n) and blocks[-1][3] == int(n.sum())
        for (a, b, r0, r1), nxt in zip(blocks, blocks[1:] + [None]):
            assert a < b and r1 - r0 == int(n[a:b].sum()) and r1 - r0 <= EC.REF_BLOCK_ROWS
            assert nxt is None or (nxt[0] == b and nxt[2] == r1)
    assert all(len(EC.node_blocks(nat)) == 1 for nat in EC.SHAPES.values())
    assert len(EC.node_blocks(EC.BIG_SHAPES["256"])) == 4 and len(EC.node_blocks(EC.BIG_SHAPES["ragged256"])) > 4
    nat = [23, 7, 1, 30]
    w = EC.layer_weights(_sd(), 0)
    frac, PQ = EC.frac_coords(nat), EC.pq("rowscale", sum(nat), 2)
    for pairs in (False, True):
        ref, b32 = EC.ref64(nat, frac, PQ, w, pairs), EC.base32(nat, frac, PQ, w, pairs)
        with monkeypatch.context() as m:
            m.setattr(EC, "REF_BLOCK_ROWS", 100)
            assert len(EC.node_blocks(nat)) > 10
            cut, cut32 = EC.ref64(nat, frac, PQ, w, pairs), EC.base32(nat, frac, PQ, w, pairs)
        assert EC.max_row_error(cut, ref) <= 2.0 ** -48
        assert EC.max_row_error(cut32, ref) <= 2 * EC.max_row_error(b32, ref)  # (another GEMM shape, the same chain)


def test_big_shape_families_stay_finite():
    nat = EC.BIG_SHAPES["81"]
    w = EC.layer_weights(_sd(), 0)
    frac = EC.frac_coords(nat)
    for family in ("normal", "rowscale"):
        PQ = EC.pq(family, sum(nat), 2)
        ref, b32 = EC.ref64(nat, frac, PQ, w, True), EC.base32(nat, frac, PQ, w, True)
        assert np.isfinite(ref).all() and np.isfinite(b32).all()
        assert EC.max_row_error(b32, ref) <= 64 * EC.U


@pytest.mark.parametrize("family", ["chunkdead", "large", "rowscale"])
def test_families_stay_finite(family):
    nat = EC.SHAPES["mixed7"]
    N = sum(nat)
    w = EC.layer_weights(_sd(), 0)
    frac = EC.frac_coords(nat)
    PQ = EC.pq(family, N, 2)
    ref, b32 = EC.ref64(nat, frac, PQ, w), EC.base32(nat, frac, PQ, w)
    assert np.isfinite(ref).all() and np.isfinite(b32).all()
    assert EC.max_row_error(b32, ref) <= 64 * EC.U
    if family == "chunkdead":
        # the dead chunk of S is exactly +-0 in fp32: a node with four dead chunks sends SiLU(b2) along every edge
        dead = np.nonzero(EC.dead_nodes(N))[0]
        assert len(dead) >= 2
        v = torch.nn.functional.silu(torch.from_numpy(w["b2"])).numpy()
        for i in dead:
            assert np.abs(b32[:, i] - v).max() <= 8 * EC.U * np.abs(v).max()
        assert np.array_equal(EC.pq(family, N, 1), PQ[:1])


def test_metric_and_gate():
    nat = [3, 5]
    w = EC.layer_weights(_sd(), 0)
    frac, PQ = EC.frac_coords(nat), EC.pq("normal", 8, 1)
    ref = EC.ref64(nat, frac, PQ, w)
    base = EC.max_row_error(EC.base32(nat, frac, PQ, w), ref)
    assert EC.U / 4 < base < 16 * EC.U
    assert EC.max_row_error(ref, ref) == 0.0
    # a per-layer error of 2^-16 in one row (what six layers and a 1e-4 parity bound would hide) fails the gate
    off = ref.copy()
    off[0, 3] *= 1 + 2.0 ** -16
    assert EC.max_row_error(off, ref) > EC.gate(base)
    # a mean divided by the wrong n
    off = ref.copy()
    off[0, 2] *= 3 / 4
    assert EC.max_row_error(off, ref) > 0.2
    bad = ref.copy()
    bad[0, 1, 7] = np.nan
    assert EC.max_row_error(bad, ref) == float("inf")
    # dead rows: must come out below DEAD
    z = np.zeros((1, 2, H))
    assert EC.max_row_error(z + 1e-31, z) == 0.0 and EC.max_row_error(z + 1e-20, z) == float("inf")


def test_split_rows_value_reads_the_layout():
    """store_split_row512's layout: per 16 columns [hi 16 | lo 16] fp16, values scaled by 2^-e per 128-column chunk."""
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, H)) * 2.0 ** rng.integers(-5, 6, (3, 4)).repeat(128, 1)).astype(np.float32)
    x[1, 128:256] = 0.0
    e = np.zeros((3, 4), np.int64)
    for c in range(4):
        m = np.abs(x[:, 128 * c:128 * c + 128]).max(1)
        e[:, c] = np.where(m > 0, np.frexp(m)[1], 0)
    xs = x * np.repeat(2.0 ** -e, 128, 1).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    split = np.stack([hi.reshape(3, H // 16, 16), lo.reshape(3, H // 16, 16)], 2)
    exps = e.astype(np.int8).view(np.int32).reshape(3)
    val, _, _, e2 = EC.split_rows_value(split, exps)
    assert np.array_equal(e2, e) and e2[1, 1] == 0
    for c in range(4):
        s = slice(128 * c, 128 * c + 128)
        assert (np.abs(val[:, s] - x[:, s]).max(1) <= 2.0 ** -22 * np.abs(x[:, s]).max(1)).all()


# ---------------------------------------------------------------- chm_debug_edge_layer refuses bad arguments (no device)

def _call(b=None, pairs=1, layer=0, frac=0x10000, n_frac=30, pq=0x20000, n_pq=None, agg=0x30000, n_agg=None,
          split=None, exp=None):
    N = n_frac // 3
    n_pq = pairs * N * 2 * H if n_pq is None else n_pq
    n_agg = pairs * N * H if n_agg is None else n_agg
    lib = _lib.load()
    rc = lib.chm_debug_edge_layer(b, pairs, layer, frac, n_frac, pq, n_pq, agg, n_agg, split, exp, None)
    return rc, lib.chm_last_error()


@pytest.mark.parametrize("kw,field", [
    (dict(frac=None), b"d_frac"), (dict(pq=None), b"d_PQ"), (dict(agg=None), b"d_agg"),
    (dict(split=0x40000), b"d_agg_exp"), (dict(exp=0x40000), b"d_agg_split"),
    (dict(pairs=0), b"pairs"), (dict(pairs=-1), b"pairs"), (dict(layer=-1), b"layer"),
    (dict(n_frac=0), b"n_frac"), (dict(n_frac=31), b"n_frac"), (dict(n_frac=-3), b"n_frac"),
    (dict(n_pq=10 * 2 * H - 1), b"n_pq"), (dict(pairs=2, n_pq=10 * 2 * H), b"n_pq"), (dict(n_pq=10 * H), b"n_pq"),
    (dict(n_agg=10 * H + 1), b"n_agg"), (dict(pairs=2, n_agg=10 * H), b"n_agg"), (dict(n_agg=0), b"n_agg"),
    (dict(frac=0x10004), b"aligned"), (dict(), b"batch"),
])
def test_debug_edge_layer_refuses_bad_arguments_without_a_device(kw, field):
    rc, err = _call(**kw)
    assert rc == -1, (kw, err)  # CHM_E_ARG, not a HIP error: no HIP call was made
    assert b"chm_debug_edge_layer" in err and field in err, (kw, err)
