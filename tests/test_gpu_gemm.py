"""The decoder's GEMM kernels one at a time (chm_debug_gemm) against a float64 reference.

Kinds: 0 gemm (fp32 MFMA), 1 gemm_bf16x3, 2 gemm_bf16x3_big, 3 node_gemm bf16x3, 4 node_gemm split16,
5 edge_gemm16's tile with the plain epilogue. Operand families, reference and metric: tests/gemm_cases.py.

Gate: eta = max_ij |C_ij - ref_ij| / (||a_i|| ||w_j||) may be 8 x the eta of a float32 CPU matmul
(torch fp32 A @ W.T) on the same operands, that baseline floored at 2^-24. Three bits of margin: split16 drops
the lo.lo term, its fp16 lo parts bottom out at 2^-25 of the row scale, and the MFMA K loop sums in a longer
sequential order than the CPU's blocked one. Every case prints its eta and baseline (pytest -s).

Guard rows: every operand is followed by 256 rows of NaN inside its own allocation and C by 8 sentinel rows, so
an over-read that reaches the arithmetic turns outputs non-finite and an over-write changes a sentinel, without
any access outside an allocation.

Found by these tests: with split16 rows scaled so that amax's exponent lands at 2^0, an amax overstated by 2^10
gave eta 76x to 705x the float32 baseline (the fp16 lo parts bottom out at 2^-25 absolute, so every factor of two
of overstatement cost one bit). node_gemm now scales the row maximum into [2^13, 2^14)
(profiles/r7/gemm_unit/README.md)."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from tests import gemm_cases as G

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
GUARD, CGUARD = 256, 8
SENT = -12345.6787109375  # C's pre-fill (exact in fp32)
MS = [1, 63, 64, 65, 127, 128, 129, 193, 257]
NS = [128, 512, 1024]
KCFG = ["512", "1024s"]  # K = 512; K = 1024 with ksplit = 512 and A2 in a second buffer (lda2 != lda)
KIND_N_MULT = {0: 128, 1: 128, 2: 256, 3: 128, 4: 128, 5: 256}


def _split(kcfg):
    """(K, ksplit or None)"""
    return (int(kcfg[:-1]), 512) if kcfg.endswith("s") else (int(kcfg), None)


@functools.lru_cache(maxsize=None)
def _ref_full(family, K):
    A, W = G.operands(family, K)
    r = G.ref64(A, None, W)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _dev_full(family, K):
    A, W = G.operands(family, K)
    return torch.tensor(A).to(DEV), torch.tensor(W).to(DEV)


@functools.lru_cache(maxsize=None)
def _baseline(family, K, M, N):
    A, W = G.operands(family, K, M, N)
    return G.baseline_eta(A, W, _ref_full(family, K)[:M, :N])


def guarded(t, rows=GUARD, pad_cols=0, fill=float("nan")):
    """t (device, [R] or [R, C]) followed by `rows` rows of `fill`, rows widened by pad_cols columns of `fill`."""
    if t.dim() == 1:
        return torch.cat([t, torch.full((rows,), fill, dtype=t.dtype, device=DEV)])
    out = torch.full((t.shape[0] + rows, t.shape[1] + pad_cols), fill, dtype=t.dtype, device=DEV)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def run_gemm(kind, A, W, A2=None, amax=None, amax2=None, bias=None, act=0, R=None, inplace_R=False, gb=None, row2g=None,
             gb_rowmod=1, gb_cols=0, tiles=(0, 0, 0), chunk_scaled=0, want_cmax=False):
    """One chm_debug_gemm call on guarded copies of the device operands. Returns C [M, N] (and cmax as float32 [M]
    when asked), after checking that C is finite and nothing past row M was written."""
    M, N = A.shape[0], W.shape[0]
    K = A.shape[1] + (A2.shape[1] if A2 is not None else 0)
    a = _lib.chm_debug_gemm_args()
    a.kind, a.act, a.M, a.N, a.K, a.chunk_scaled = kind, act, M, N, K, chunk_scaled
    keep = []

    def dev(t, **kw):
        keep.append(guarded(t, **kw))
        return keep[-1]

    dA = dev(A)
    a.d_A, a.lda = dA.data_ptr(), dA.shape[1]
    if A2 is not None:
        dA2 = dev(A2, pad_cols=8)
        a.d_A2, a.lda2, a.ksplit = dA2.data_ptr(), dA2.shape[1], A.shape[1]
    a.d_W = dev(W).data_ptr()
    if amax is not None:
        a.d_amax = dev(amax).data_ptr()
    if amax2 is not None:
        a.d_amax2 = dev(amax2).data_ptr()
    if bias is not None:
        a.d_bias = dev(bias).data_ptr()
    dC = torch.full((M + CGUARD, N), SENT, dtype=torch.float32, device=DEV)
    if inplace_R:  # C == R: the residual is C's old content
        dC[:M] = R
        a.d_R, a.ldr = dC.data_ptr(), N
    elif R is not None:
        dR = dev(R)
        a.d_R, a.ldr = dR.data_ptr(), N
    if gb is not None:
        dgb = dev(gb, pad_cols=4)
        a.d_gb, a.ldgb, a.gb_cols, a.gb_rowmod = dgb.data_ptr(), dgb.shape[1], gb_cols, gb_rowmod
        a.d_row2g = dev(row2g, fill=0).data_ptr()
    a.d_C, a.ldc = dC.data_ptr(), N
    a.tile_rows, a.tile_cols, a.blocks_per_cu = tiles
    cmax = None
    if want_cmax:
        cmax = torch.zeros(M + GUARD, dtype=torch.int32, device=DEV)
        a.d_cmax = cmax.data_ptr()
    lib = _lib.load()
    rc = lib.chm_debug_gemm(ctypes.byref(a), _lib.stream_handle())
    if rc == -2:  # a HIP error (a fault included): nothing more may run on this device in this session
        pytest.exit(f"chm_debug_gemm: {lib.chm_last_error().decode(errors='replace')}", returncode=3)
    assert rc == 0, lib.chm_last_error()
    torch.cuda.synchronize()
    C = dC[:M]
    assert bool(torch.isfinite(C).all()), "non-finite outputs: a guard row reached the arithmetic"
    assert torch.equal(dC[M:].view(torch.int32), torch.full((CGUARD, N), SENT, device=DEV).view(torch.int32)), \
        "rows past M were written"
    if want_cmax:
        assert not bool(cmax[M:].any()), "cmax past row M was written"
        return C, cmax[:M].view(torch.float32)
    return C


def case_operands(family, kcfg, M, N):
    """Device operands (A, A2 or None, W) of a case and its float64 reference and host operands."""
    K, ks = _split(kcfg)
    dA, dW = _dev_full(family, K)
    hA, hW = G.operands(family, K, M, N)
    A, A2 = (dA[:M, :ks], dA[:M, ks:]) if ks else (dA[:M], None)
    return A, A2, dW[:N], hA, hW, _ref_full(family, K)[:M, :N]


def check_eta(tag, C, family, K, M, N, hA, hW, ref):
    e, base = G.eta(C.cpu().numpy(), hA, hW, ref), _baseline(family, K, M, N)
    print(f"{tag}: eta {e:.3e} baseline {base:.3e} ratio {e / base:.2f}")
    assert e <= G.GATE_FACTOR * base, f"{tag}: eta {e:.3e} above 8 x the float32 baseline {base:.3e}"


# ---------------------------------------------------------------- accuracy against float64

# kinds 0-4 on every family, K configuration, N and M; the bf16x3 kernels also at K = 640 (the conditioning GEMM)
ACCURACY = [(kind, f, k, n, m) for kind in range(5) for f in G.FAMILIES
            for k in KCFG + (["640"] if kind in (1, 2, 3) else []) for n in NS for m in MS]


@pytest.mark.parametrize("kind,family,kcfg,N,M", ACCURACY)
def test_accuracy(kind, family, kcfg, N, M):
    A, A2, W, hA, hW, ref = case_operands(family, kcfg, M, N)
    K = hA.shape[1]
    if N % KIND_N_MULT[kind]:  # (gemm_bf16x3_big has 256-column tiles: the hook must refuse, not run)
        a = _lib.chm_debug_gemm_args()
        a.kind, a.M, a.N, a.K = kind, M, N, K
        a.d_A, a.lda, a.d_W, a.d_C, a.ldc = A.data_ptr(), K, W.data_ptr(), A.data_ptr(), N
        lib = _lib.load()
        assert lib.chm_debug_gemm(ctypes.byref(a), None) == -1 and b"N" in lib.chm_last_error()
        return
    amax = amax2 = None
    if kind == 4:  # the exact row maxima (zerorows: 0 for the zero rows, whose outputs must be exactly 0)
        amax = A.abs().amax(1)
        amax2 = A2.abs().amax(1) if A2 is not None else None
    C = run_gemm(kind, A, W, A2, amax, amax2)
    check_eta(f"kind {kind} {family} K={kcfg} N={N} M={M}", C, family, K, M, N, hA, hW, ref)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kcfg", KCFG)
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("over", [3.0, 1024.0], ids=["x3", "x2^10"])
def test_accuracy_split16_amax_upper_bound(over, family, kcfg, N, M):
    """amax that is only an upper bound of the row maximum: the row scale puts amax's exponent at 2^14, so ten bits
    of overstatement still leave the fp16 lo parts at fp32 level."""
    A, A2, W, hA, hW, ref = case_operands(family, kcfg, M, N)
    amax = A.abs().amax(1) * over
    amax2 = A2.abs().amax(1) * over if A2 is not None else None
    C = run_gemm(4, A, W, A2, amax, amax2)
    check_eta(f"kind 4 amax {over:g}x {family} K={kcfg} N={N} M={M}", C, family, hA.shape[1], M, N, hA, hW, ref)


@pytest.mark.parametrize("big", ["A2", "A"])
@pytest.mark.parametrize("kind", [3, 4])
def test_row_scale_covers_both_halves(kind, big):
    """Node MLP 1 reads [h | agg], two buffers of different magnitude: one half 2^20 times the other. The row's
    scale must come from max(amax, amax2): from amax alone the larger half leaves the fp16 range."""
    M, N = 129, 512
    A, A2, W, hA, hW, _ = case_operands("normal", "1024s", M, N)
    f = np.float32(2.0 ** 20)
    hA = hA.copy()
    if big == "A2":
        A2, hA[:, 512:] = A2 * f, hA[:, 512:] * f
    else:
        A, hA[:, :512] = A * f, hA[:, :512] * f
    am, am2 = (A.abs().amax(1), A2.abs().amax(1)) if kind == 4 else (None, None)
    C = run_gemm(kind, A, W, A2, am, am2)
    ref = G.ref64(hA, None, hW)
    e, base = G.eta(C.cpu().numpy(), hA, hW, ref), G.baseline_eta(hA, hW, ref)
    print(f"kind {kind} {big} x 2^20: eta {e:.3e} baseline {base:.3e} ratio {e / base:.2f}")
    assert e <= G.GATE_FACTOR * base


def test_split16_unscaled_rows_below_one():
    """amax = NULL: rows are split as they are (the contract then is |a| <= 1, as for the Fourier features)."""
    A, _, W, hA, hW, ref = case_operands("normal", "512", 129, 512)
    s = float(np.abs(hA).max()) * 1.01
    A, hA, ref = A / s, (hA / np.float32(s)).astype(np.float32), None
    C = run_gemm(4, A, W)
    e, base = G.eta(C.cpu().numpy(), hA, hW), G.baseline_eta(hA, hW)
    print(f"kind 4 unscaled: eta {e:.3e} baseline {base:.3e}")
    assert e <= G.GATE_FACTOR * base


@functools.lru_cache(maxsize=None)
def _edge_case(family, K):
    A, W = G.operands(family, K, G.M_MAX, 512)
    if K == 768:  # layer 1's A operand is Fourier features: |a| <= 1
        A = np.clip(A, -1.0, 1.0)
    A = np.concatenate([A, A[:385 - G.M_MAX][::-1] * np.float32(0.5)])  # 385 rows
    ref = G.ref64(A, None, W)
    return A, W, ref, torch.tensor(A).to(DEV), torch.tensor(W).to(DEV)


@pytest.mark.parametrize("M", [1, 255, 256, 257, 385])
@pytest.mark.parametrize("family,K,chunk_scaled", [("normal", 768, 0), ("widerow", 768, 0), ("normal", 512, 1),
                                                   ("widerow", 512, 1), ("spike", 512, 1)])
def test_accuracy_edge_tile(family, K, chunk_scaled, M):
    """Kind 5: K = 768, N = 512 is edge layer 1 (unscaled A, clipped to |a| <= 1), K = 512 with chunk-scaled A is
    edge layer 2."""
    hA, hW, ref, dA, dW = _edge_case(family, K)
    C = run_gemm(5, dA[:M], dW, chunk_scaled=chunk_scaled)
    e, base = G.eta(C.cpu().numpy(), hA[:M], hW, ref[:M]), G.baseline_eta(hA[:M], hW, ref[:M])
    print(f"kind 5 {family} K={K} chunk_scaled={chunk_scaled} M={M}: eta {e:.3e} baseline {base:.3e} ratio {e / base:.2f}")
    assert e <= G.GATE_FACTOR * base


# ---------------------------------------------------------------- epilogue

EPI_CASES = ["bias", "bias_silu", "silu_R_inplace", "gb", "bias_gb_silu_R", "A2_bias_silu"]


def epilogue_inputs(case, N, seed=0):
    """(M, kcfg, host dict of bias / R / gb / row2g / gb_rowmod / gb_cols / act) of an epilogue case."""
    rng = np.random.default_rng([seed, N, EPI_CASES.index(case)])
    M = 120 if "gb" in case else 129  # gb: P = 2 conditionings x 60 nodes, 3 graphs
    h = dict(act=int("silu" in case))
    if "bias" in case:
        h["bias"] = rng.standard_normal(N).astype(np.float32)
    if "R" in case:
        h["R"] = rng.standard_normal((M, N)).astype(np.float32)
    if "gb" in case:
        h["gb"] = rng.standard_normal((3, N // 2)).astype(np.float32)
        h["row2g"] = np.repeat(np.arange(3, dtype=np.int32), [13, 20, 27])
        h["gb_rowmod"], h["gb_cols"] = 60, N // 2  # (512 of N = 1024: columns >= gb_cols receive no gb)
    return M, ("1024s" if case.startswith("A2") else "512"), h


def run_epilogue(kind, case, N, tiles=(0, 0, 0), want_cmax=False, family="normal"):
    M, kcfg, h = epilogue_inputs(case, N)
    A, A2, W, hA, hW, _ = case_operands(family, kcfg, M, N)
    d = {k: torch.tensor(v).to(DEV) for k, v in h.items() if isinstance(v, np.ndarray)}
    amax = A.abs().amax(1) if kind == 4 else None
    amax2 = A2.abs().amax(1) if kind == 4 and A2 is not None else None
    out = run_gemm(kind, A, W, A2, amax, amax2, bias=d.get("bias"), act=h["act"], R=d.get("R"),
                   inplace_R="inplace" in case, gb=d.get("gb"), row2g=d.get("row2g"), gb_rowmod=h.get("gb_rowmod", 1),
                   gb_cols=h.get("gb_cols", 0), tiles=tiles, want_cmax=want_cmax)
    return out, (M, kcfg, h, hA, hW)


@functools.lru_cache(maxsize=None)
def silu_c(case, N):
    """c of the tolerance's c u |ref| term. SiLU cases: 4 x the error (in u |ref|) of a float32
    torch.nn.functional.silu applied to the float64 pre-activation, at most 16: the kernels' v_exp / v_rcp SiLU
    may cost that much more than a float32 libm one. Without SiLU the epilogue is at most three fp32 additions
    (bias, gb, R), one rounding each: c = 4 with one to spare."""
    M, kcfg, h = epilogue_inputs(case, N)
    if not h["act"]:
        return 4.0, 0.0
    K, ks = _split(kcfg)
    hA, hW = G.operands("normal", K, M, N)
    Z = G.preact64(hA, None, hW, h.get("bias"), h.get("gb"), h.get("row2g"), h.get("gb_rowmod", 1), h.get("gb_cols", 0))
    s32 = torch.nn.functional.silu(torch.tensor(Z).float()).double().numpy()
    s64 = G.silu64(Z)
    base = float((np.abs(s32 - s64) / (G.U * np.abs(s64))).max())
    return min(4.0 * base, 16.0), base


@pytest.mark.parametrize("N", [1024, 512])
@pytest.mark.parametrize("case", EPI_CASES)
@pytest.mark.parametrize("kind", [0, 3, 4])
def test_epilogue(kind, case, N):
    """|err_ij| <= 1.1 gate_eta ||a_i|| ||w_j|| + c u |ref_ij|: 1.1 is SiLU's Lipschitz bound on the GEMM's own
    error, c u |ref| the epilogue's rounding (silu_c)."""
    C, (M, kcfg, h, hA, hW) = run_epilogue(kind, case, N)
    ref = G.ref64(hA, None, hW, h.get("bias"), h.get("gb"), h.get("row2g"), h.get("gb_rowmod", 1), h.get("gb_cols", 0),
                  h["act"], h.get("R"))
    na, nw = G.norms(hA, hW)
    c, c_base = silu_c(case, N)
    gate_eta = G.GATE_FACTOR * _baseline("normal", hA.shape[1], M, N)
    tol = 1.1 * gate_eta * np.outer(na, nw) + c * G.U * np.abs(ref)
    err = np.abs(C.cpu().numpy().astype(np.float64) - ref)
    print(f"kind {kind} {case} N={N}: max err/tol {float((err / tol).max()):.3f}, max err {float(err.max()):.3e}, "
          f"c {c:.2f} (float32 silu: {c_base:.2f})")
    assert (err <= tol).all(), f"max err / tol {float((err / tol).max()):.2f}"
    if "gb" in case:  # columns >= gb_cols: exactly the call without gb
        C0, _ = run_epilogue_without_gb(kind, case, N)
        assert torch.equal(C[:, h["gb_cols"]:], C0[:, h["gb_cols"]:])
        assert not torch.equal(C[:, :h["gb_cols"]], C0[:, :h["gb_cols"]])


def run_epilogue_without_gb(kind, case, N):
    M, kcfg, h = epilogue_inputs(case, N)
    A, A2, W, _, _, _ = case_operands("normal", kcfg, M, N)
    d = {k: torch.tensor(v).to(DEV) for k, v in h.items() if isinstance(v, np.ndarray)}
    amax = A.abs().amax(1) if kind == 4 else None
    return run_gemm(kind, A, W, A2, amax, None, bias=d.get("bias"), act=h["act"], R=d.get("R")), None


# ---------------------------------------------------------------- cmax

@pytest.mark.parametrize("tiles", [(0, 0, 0), (64, 128, 3), (128, 128, 3)], ids=["default", "64x128", "128x128"])
@pytest.mark.parametrize("case", [None, "bias_gb_silu_R", "A2_bias_silu"])
@pytest.mark.parametrize("family", ["normal", "rowscale"])
def test_cmax_is_the_output_row_maximum(family, case, tiles):
    """cmax sets the next GEMM's row scale: bit for bit max |C[row, :]| of what was stored."""
    if case is None:
        A, _, W, _, _, _ = case_operands(family, "512", 129, 512)
        C, cmax = run_gemm(4, A, W, amax=A.abs().amax(1), tiles=tiles, want_cmax=True)
    else:
        (C, cmax), _ = run_epilogue(4, case, 1024, tiles=tiles, want_cmax=True, family=family)
    assert torch.equal(cmax.view(torch.int32), C.abs().amax(1).view(torch.int32))


# ---------------------------------------------------------------- bit-identity of the tile variants, M-independence

S16_TILES = [(64, 64, 0), (64, 128, 3), (64, 128, 4), (128, 128, 3), (128, 128, 2)]


@pytest.mark.parametrize("N", [512, 1024])
@pytest.mark.parametrize("M", [65, 193, 257])
@pytest.mark.parametrize("family", ["normal", "widerow", "spike"])
def test_split16_tile_variants_are_bit_identical(family, M, N):
    A, _, W, _, _, _ = case_operands(family, "512", M, N)
    amax = A.abs().amax(1)
    outs = [run_gemm(4, A, W, amax=amax, tiles=t) for t in S16_TILES]
    for t, o in zip(S16_TILES[1:], outs[1:]):
        assert torch.equal(outs[0], o), f"tiles {t} differ from {S16_TILES[0]}"
    assert torch.equal(outs[0], run_gemm(4, A, W, amax=amax)), "the default choice differs"


@pytest.mark.parametrize("case", ["bias_gb_silu_R", "A2_bias_silu", "silu_R_inplace", "gb"])
def test_split16_tile_variants_are_bit_identical_with_epilogue(case):
    """(the 64-row tiles load their epilogue vectors ahead of the K loop, the 64x64 ones also the residual rows)"""
    outs = [run_epilogue(4, case, 1024, tiles=t)[0] for t in S16_TILES]
    for t, o in zip(S16_TILES[1:], outs[1:]):
        assert torch.equal(outs[0], o), f"tiles {t} differ from {S16_TILES[0]}"


@pytest.mark.parametrize("N", [512, 1024])
@pytest.mark.parametrize("M", [65, 193, 257])
@pytest.mark.parametrize("family", ["normal", "widerow", "spike"])
def test_bf16x3_node_tile_rows_are_bit_identical(family, M, N):
    A, _, W, _, _, _ = case_operands(family, "512", M, N)
    assert torch.equal(run_gemm(3, A, W, tiles=(64, 0, 0)), run_gemm(3, A, W, tiles=(128, 0, 0)))


@pytest.mark.parametrize("family", ["normal", "widerow", "rowscale"])
@pytest.mark.parametrize("kcfg", KCFG)
@pytest.mark.parametrize("kind", [3, 4])
def test_rows_do_not_depend_on_M(kind, kcfg, family):
    """What keeps a sharded run bit-identical to one process: a row's result is the same in an M = 257 call,
    alone (M = 1) and as one of four rows (M = 4), with the same amax."""
    rows = [0, 64, 192, 256]
    A, A2, W, _, _, _ = case_operands(family, kcfg, 257, 512)
    am = A.abs().amax(1) if kind == 4 else None
    am2 = A2.abs().amax(1) if kind == 4 and A2 is not None else None
    sel = lambda t, r: None if t is None else t[r].contiguous()  # noqa: E731
    full = run_gemm(kind, A, W, A2, am, am2)
    four = run_gemm(kind, sel(A, rows), W, sel(A2, rows), sel(am, rows), sel(am2, rows))
    assert torch.equal(full[rows], four), "rows of the M = 257 call differ from the M = 4 call"
    for k, r in enumerate(rows):
        one = run_gemm(kind, sel(A, [r]), W, sel(A2, [r]), sel(am, [r]), sel(am2, [r]))
        assert torch.equal(full[r:r + 1], one), f"row {r}: M = 257 differs from M = 1"
