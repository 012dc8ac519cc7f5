"""CPU checks of the GEMM test harness (tests/gemm_cases.py) and of chm_debug_gemm's argument checks.

The gate of tests/test_gpu_gemm.py (eta <= 8 x the float32 CPU matmul's eta, floored at 2^-24) must be one the
kernels' arithmetic can meet and a broken arithmetic cannot: numpy models of split16 (fp16 hi/lo, three products)
and bf16x3 (three bf16 parts, six products) pass it on every operand family, and the same models with their
low-order terms dropped fail it. chm_debug_gemm refuses bad arguments with CHM_E_ARG naming the field before any
HIP call, so those checks run here without a device."""

import ctypes

import numpy as np
import pytest

from chemeleon_amd import _lib
from tests import gemm_cases as G

M, N = 193, 128


@pytest.mark.parametrize("K", [512, 1024])
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("model", ["split16", "bf16x3"])
def test_model_meets_the_gate(model, family, K):
    A, W = G.operands(family, K, M, N)
    ref = G.ref64(A, None, W)
    C = G.model_split16(A, W) if model == "split16" else G.model_bf16x3(A, W)
    e, base = G.eta(C, A, W, ref), G.baseline_eta(A, W, ref)
    print(f"{model} {family} K={K}: eta {e:.3e} baseline {base:.3e} ratio {e / base:.2f}")
    assert e <= G.GATE_FACTOR * base
    if family == "zerorows":
        assert not C[::7].any()


@pytest.mark.parametrize("family", G.FAMILIES)
def test_split16_model_under_an_amax_that_is_an_upper_bound(family):
    """The fp16 lo parts bottom out at 2^-25 absolute. With the row maximum scaled into [2^13, 2^14) an amax
    overstated 3x or 2^10 x still meets the gate; scaled into [0.5, 1) (a_up = 0) the 2^10 x case loses ten bits."""
    A, W = G.operands(family, 512, M, N)
    ref = G.ref64(A, None, W)
    g = G.gate(A, W, ref)
    for over in (3.0, 1024.0):
        assert G.eta(G.model_split16(A, W, G.row_amax(A) * np.float32(over)), A, W, ref) <= g, over
    assert G.eta(G.model_split16(A, W, G.row_amax(A) * np.float32(1024.0), a_up=0), A, W, ref) > g


@pytest.mark.parametrize("family", ["normal", "widerow"])
def test_gate_refuses_a_two_product_split(family):
    """hi.hi alone (fp16) or the three leading bf16 products lose 2^-11 / 2^-16 relative: far outside the gate."""
    A, W = G.operands(family, 512, M, N)
    ref = G.ref64(A, None, W)
    sa, sw = G._frexp_scale(G.row_amax(A))[:, None], G._frexp_scale(G.row_amax(W))[:, None]
    ah = (A / sa).astype(np.float16).astype(np.float32)
    wh = (W / sw).astype(np.float16).astype(np.float32)
    assert G.eta((ah @ wh.T) * (sw.T * sa), A, W, ref) > G.gate(A, W, ref)
    a0, w0 = G._bf16(A), G._bf16(W)
    a1, w1 = G._bf16(A - a0), G._bf16(W - w0)
    assert G.eta(a0 @ w0.T + a0 @ w1.T + a1 @ w0.T, A, W, ref) > G.gate(A, W, ref)


def test_operand_families_are_what_they_say():
    for f in G.FAMILIES:
        A, W = G.operands(f, 512)
        assert A.shape == (G.M_MAX, 512) and W.shape == (G.N_MAX, 512) and A.dtype == np.float32
        assert np.isfinite(A).all() and np.isfinite(W).all()
        A2, W2 = G.operands(f, 512, 65, 128)
        assert np.array_equal(A2, A[:65]) and np.array_equal(W2, W[:128])  # rows do not depend on M, N
    A, W = G.operands("pos", 512)
    assert (A >= 0).all() and (W >= 0).all()
    A, _ = G.operands("zerorows", 512)
    assert not A[::7].any() and A[1::7].any() and (G.row_amax(A)[::7] == 0).all()
    A, W = G.operands("spike", 512)
    assert ((A == 100).sum(1) == 1).all() and ((W == 100).sum(1) == 1).all() and np.abs(A[A != 100]).max() < 1e-3
    A, W = G.operands("rowscale", 512)
    ra = np.log2(G.row_amax(A))
    assert ra.max() - ra.min() > 60
    A, _ = G.operands("widerow", 512)
    assert (np.log2(G.row_amax(A) / np.abs(A).min(1).clip(1e-300)) > 24).all()


def test_eta_and_ref64():
    A, W = G.operands("zerorows", 512, 15, 128)
    ref = G.ref64(A, None, W)
    assert G.eta(ref, A, W) == 0.0
    C = ref.copy()
    C[0, 3] = 1e-30  # a zero row must be exactly zero
    assert G.eta(C, A, W) == float("inf")
    C = ref.copy()
    C[1, 0] = np.nan
    assert G.eta(C, A, W) == float("inf")
    C = ref.copy()
    C[1, 5] += 1e-3
    na, nw = G.norms(A, W)
    assert G.eta(C, A, W) == pytest.approx(1e-3 / (na[1] * nw[5]), rel=1e-6)
    # the epilogue: bias, per-graph row bias on the first gb_cols columns, SiLU, then the residual
    rng = np.random.default_rng(0)
    bias, gb, R = rng.standard_normal(128), rng.standard_normal((3, 64)), rng.standard_normal((15, 128))
    row2g = np.array([0, 1, 2, 2, 1])
    Z = A.astype(np.float64) @ W.astype(np.float64).T + bias
    Z[:, :64] += gb[row2g[np.arange(15) % 5]]
    want = Z / (1 + np.exp(-Z)) + R
    got = G.ref64(A, None, W, bias, gb, row2g, 5, 64, 1, R)
    assert np.array_equal(got, want)
    A1, A2 = A[:, :256], A[:, 256:]
    np.testing.assert_allclose(G.ref64(A1, A2, W), ref, rtol=0, atol=0)


# ---------------------------------------------------------------- chm_debug_gemm refuses bad arguments (no device)

def _args(**kw):
    """A well-formed call on fake (never dereferenced) device pointers."""
    a = _lib.chm_debug_gemm_args()
    a.kind, a.M, a.N, a.K = 4, 65, 512, 512
    a.d_A, a.lda, a.d_W, a.d_C, a.ldc = 0x10000, 512, 0x20000, 0x30000, 512
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD = [
    (dict(kind=6), b"kind"), (dict(kind=-1), b"kind"), (dict(M=0), b"M"), (dict(N=0), b"N"), (dict(K=-16), b"K"),
    (dict(d_A=None), b"d_A"), (dict(d_W=None), b"d_W"), (dict(d_C=None), b"d_C"), (dict(act=2), b"act"),
    (dict(N=192), b"N"), (dict(kind=2, N=128), b"N"), (dict(kind=5, N=128), b"N"),
    (dict(K=528), b"K"), (dict(kind=0, K=520), b"K"), (dict(kind=5, K=544), b"K"), (dict(kind=1, K=528), b"K"),
    (dict(ksplit=256), b"ksplit"), (dict(d_A2=0x40000, lda2=256, ksplit=8), b"ksplit"),
    (dict(d_A2=0x40000, lda2=256, ksplit=512), b"ksplit"), (dict(d_A2=0x40000, lda2=128, ksplit=256), b"lda2"),
    (dict(d_A2=0x40000, lda2=258, ksplit=256), b"lda2"), (dict(kind=5, d_A2=0x40000, lda2=256, ksplit=256), b"d_A2"),
    (dict(lda=511), b"lda"), (dict(lda=514), b"lda"), (dict(ldc=256), b"ldc"), (dict(ldc=514), b"ldc"),
    (dict(d_R=0x50000, ldr=8), b"ldr"),
    (dict(kind=2, d_gb=0x50000, ldgb=512, gb_cols=512, d_row2g=0x60000, gb_rowmod=1), b"d_gb"),
    (dict(d_gb=0x50000, ldgb=512, gb_cols=512, gb_rowmod=1), b"d_row2g"),
    (dict(d_gb=0x50000, ldgb=512, gb_cols=512, d_row2g=0x60000, gb_rowmod=0), b"gb_rowmod"),
    (dict(d_gb=0x50000, ldgb=512, gb_cols=1024, d_row2g=0x60000, gb_rowmod=1), b"gb_cols"),
    (dict(d_gb=0x50000, ldgb=512, gb_cols=6, d_row2g=0x60000, gb_rowmod=1), b"gb_cols"),
    (dict(d_gb=0x50000, ldgb=256, gb_cols=512, d_row2g=0x60000, gb_rowmod=1), b"ldgb"),
    (dict(kind=5, d_bias=0x50000), b"d_bias"), (dict(kind=5, act=1), b"act"), (dict(kind=5, d_R=0x50000, ldr=512), b"d_R"),
    (dict(chunk_scaled=1), b"chunk_scaled"), (dict(kind=5, chunk_scaled=2), b"chunk_scaled"),
    (dict(kind=5, K=768, lda=768, chunk_scaled=1), b"chunk_scaled"),
    (dict(kind=5, K=576, lda=576, chunk_scaled=1), b"chunk_scaled"),
    (dict(kind=3, d_cmax=0x70000), b"d_cmax"), (dict(kind=0, d_cmax=0x70000), b"d_cmax"),
    (dict(kind=1, tile_rows=64), b"tile_rows"), (dict(kind=0, blocks_per_cu=2), b"blocks_per_cu"),
    (dict(kind=5, tile_cols=64), b"tile_cols"), (dict(tile_rows=32), b"tile_rows"), (dict(tile_rows=256), b"tile_rows"),
    (dict(kind=3, tile_rows=64, tile_cols=64), b"tile_cols"), (dict(kind=3, tile_rows=64, blocks_per_cu=3), b"blocks_per_cu"),
    (dict(tile_rows=64, tile_cols=32), b"tile_cols"), (dict(tile_rows=128, tile_cols=64), b"tile_cols"),
    (dict(tile_cols=64), b"tile_cols"), (dict(blocks_per_cu=3), b"blocks_per_cu"),
    (dict(tile_rows=64, tile_cols=128, blocks_per_cu=5), b"blocks_per_cu"),
    (dict(tile_rows=64, tile_cols=128, blocks_per_cu=2), b"blocks_per_cu"),
    (dict(tile_rows=64, tile_cols=64, blocks_per_cu=3), b"blocks_per_cu"),
    (dict(tile_rows=64, blocks_per_cu=3), b"blocks_per_cu"),
    (dict(tile_rows=128, blocks_per_cu=4), b"blocks_per_cu"),
    (dict(d_A=0x10004), b"aligned"), (dict(d_C=0x30008), b"aligned"),
]


@pytest.mark.parametrize("kw,field", BAD, ids=[f"{i}-{f.decode()}" for i, (_, f) in enumerate(BAD)])
def test_debug_gemm_refuses_bad_arguments_without_a_device(kw, field):
    lib = _lib.load()
    rc = lib.chm_debug_gemm(ctypes.byref(_args(**kw)), None)
    err = lib.chm_last_error()
    assert rc == -1, (kw, err)  # CHM_E_ARG, not a HIP error: no HIP call was made
    assert b"chm_debug_gemm" in err and field in err, (kw, err)


def test_debug_gemm_refuses_null_args():
    lib = _lib.load()
    assert lib.chm_debug_gemm(None, None) == -1 and b"NULL" in lib.chm_last_error()
