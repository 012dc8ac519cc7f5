"""Operand families, the float64 reference and the error metric of the per-kernel GEMM tests
(tests/test_gemm_cases.py on the CPU, tests/test_gpu_gemm.py on the GPU). A plain helper module: every
family is seeded, every function is pure numpy.

C[M, N] = epi(A[M, K] . W[N, K]^T), the decoder's GEMM (include/chemeleon_hip.h, chm_debug_gemm)."""

import functools

import numpy as np

FAMILIES = ("normal", "pos", "widerow", "rowscale", "spike", "zerorows")
U = 2.0 ** -24          # fp32 unit roundoff
GATE_FACTOR = 8.0       # the kernels' eta may be this many times the float32 CPU matmul's (floored at U)
M_MAX, N_MAX = 257, 1024


def _rng(family, K, what):
    return np.random.default_rng([FAMILIES.index(family), K, what])


@functools.lru_cache(maxsize=None)
def operands(family, K, M=M_MAX, N=N_MAX):
    """(A [M, K], W [N, K]) float32, read-only. Rows do not depend on M or N: operands(f, K, m, n) are the
    first m / n rows of operands(f, K)."""
    if (M, N) != (M_MAX, N_MAX):
        A, W = operands(family, K)
        return A[:M], W[:N]
    ra, rw = _rng(family, K, 0), _rng(family, K, 1)
    A = ra.standard_normal((M, K))
    W = 0.05 * rw.standard_normal((N, K))
    if family == "pos":
        A, W = np.abs(A), np.abs(W)
    elif family == "widerow":  # a wide dynamic range inside every row
        A = A * 2.0 ** ra.uniform(-24, 0, A.shape)
        W = W * 2.0 ** rw.uniform(-24, 0, W.shape)
    elif family == "rowscale":  # rows far apart in scale
        A = A * 2.0 ** ra.integers(-40, 40, (M, 1))
        W = W * 2.0 ** rw.integers(-30, 30, (N, 1))
    elif family == "spike":  # one element dominates the row
        A = 1e-4 * ra.standard_normal((M, K))
        W = 1e-4 * rw.standard_normal((N, K))
        A[np.arange(M), ra.integers(0, K, M)] = 100.0
        W[np.arange(N), rw.integers(0, K, N)] = 100.0
    elif family == "zerorows":
        A[::7] = 0.0
    A, W = A.astype(np.float32), W.astype(np.float32)
    A.setflags(write=False)
    W.setflags(write=False)
    return A, W


def row_amax(A):
    """max |A[row, :]| per row, float32 (0 for a zero row): the split16 node GEMM's amax."""
    return np.abs(A).max(axis=1).astype(np.float32)


def silu64(x):
    return x / (1.0 + np.exp(-x))


def preact64(A, A2, W, bias=None, gb=None, row2g=None, gb_rowmod=1, gb_cols=0):
    """The float64 pre-activation: [A | A2] . W^T + bias + the per-graph row bias on columns < gb_cols."""
    Af = np.asarray(A, np.float64) if A2 is None else np.concatenate([np.asarray(A, np.float64), np.asarray(A2, np.float64)], 1)
    Z = Af @ np.asarray(W, np.float64).T
    if bias is not None:
        Z = Z + np.asarray(bias, np.float64)[None, :]
    if gb is not None:
        rows = np.asarray(row2g)[np.arange(Z.shape[0]) % gb_rowmod]
        Z[:, :gb_cols] += np.asarray(gb, np.float64)[rows, :gb_cols]
    return Z


def ref64(A, A2, W, bias=None, gb=None, row2g=None, gb_rowmod=1, gb_cols=0, act=0, R=None):
    """The float64 reference of the whole call. SiLU is x / (1 + exp(-x)); R (the residual) is added after it."""
    Z = preact64(A, A2, W, bias, gb, row2g, gb_rowmod, gb_cols)
    if act == 1:
        Z = silu64(Z)
    if R is not None:
        Z = Z + np.asarray(R, np.float64)
    return Z


def norms(A, W, A2=None):
    """(||a_i||_2 [M], ||w_j||_2 [N]) in float64, a_i the whole row [A | A2]."""
    na2 = (np.asarray(A, np.float64) ** 2).sum(1)
    if A2 is not None:
        na2 = na2 + (np.asarray(A2, np.float64) ** 2).sum(1)
    return np.sqrt(na2), np.sqrt((np.asarray(W, np.float64) ** 2).sum(1))


def eta(C, A, W, ref=None, A2=None):
    """Normwise error of C against the float64 product: max_ij |C_ij - ref_ij| / (||a_i|| ||w_j||). Rows and
    columns of zero norm must be exactly 0 in C (else the result is inf). NaN / inf in C give inf."""
    C = np.asarray(C, np.float64)
    if ref is None:
        ref = ref64(A, A2, W)
    na, nw = norms(A, W, A2)
    if not np.isfinite(C).all():
        return float("inf")
    za, zw = na == 0, nw == 0
    if (C[za] != 0).any() or (C[:, zw] != 0).any():
        return float("inf")
    den = np.outer(np.where(za, 1.0, na), np.where(zw, 1.0, nw))
    err = np.abs(C - ref) / den
    err[za] = 0.0
    err[:, zw] = 0.0
    return float(err.max()) if err.size else 0.0


def baseline_eta(A, W, ref=None, A2=None):
    """eta of the float32 CPU matmul (torch fp32 A @ W.T) on the same operands, floored at U."""
    import torch
    Af = A if A2 is None else np.concatenate([A, A2], 1)
    C32 = (torch.tensor(np.asarray(Af, np.float32)) @ torch.tensor(np.asarray(W, np.float32)).T).numpy()
    return max(eta(C32, A, W, ref, A2), U)


def gate(A, W, ref=None, A2=None):
    return GATE_FACTOR * baseline_eta(A, W, ref, A2)


# ---------------------------------------------------------------- numpy models of the two split arithmetics

def _bf16(x):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((b >> 16) & 1) + np.uint32(0x7FFF)
    return ((b + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _frexp_scale(m):
    """2^e per row, e the frexp exponent of m (m = f 2^e, f in [0.5, 1); e = 0 for m == 0): float32, exact."""
    _, e = np.frexp(np.asarray(m, np.float32))
    e = np.where(np.asarray(m) > 0, e, 0)
    return np.ldexp(np.float32(1.0), e).astype(np.float32)


def model_split16(A, W, amax=None, a_up=14):
    """The split16 node GEMM in numpy: rows of A scaled by 2^(a_up - e) (e from amax, default the exact row maxima;
    a_up = 14 as in node_gemm.hip: the maximum at the top of the fp16 range), rows of W by 2^-e of their maxima;
    hi = fp16(x), lo = fp16(x - hi); per 16-deep K-tile the three products lo.hi, hi.lo, hi.hi accumulated in
    fp32 in that order; the scales undone at the end."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    sa = (_frexp_scale(row_amax(A) if amax is None else amax) * np.float32(2.0 ** -a_up))[:, None]
    sw = _frexp_scale(row_amax(W))[:, None]
    xa, xw = A / sa, W / sw  # (exact: powers of two)
    ah = xa.astype(np.float16).astype(np.float32)
    al = (xa - ah).astype(np.float16).astype(np.float32)
    wh = xw.astype(np.float16).astype(np.float32)
    wl = (xw - wh).astype(np.float16).astype(np.float32)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in range(0, A.shape[1], 16):
        s = slice(k, k + 16)
        acc = acc + al[:, s] @ wh[:, s].T
        acc = acc + ah[:, s] @ wl[:, s].T
        acc = acc + ah[:, s] @ wh[:, s].T
    return acc * (sw.T * sa)


def model_bf16x3(A, W):
    """bf16x3 in numpy: x = x0 + x1 + x2 (bf16 parts), per 16-deep K-tile the six products of weight >= 2^-16
    (a2w0, a1w1, a0w2, a1w0, a0w1, a0w0: small terms first) accumulated in fp32."""
    def parts(x):
        x = np.asarray(x, np.float32)
        p0 = _bf16(x)
        p1 = _bf16(x - p0)
        return p0, p1, _bf16(x - p0 - p1)
    a, w = parts(A), parts(W)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in range(0, A.shape[1], 16):
        s = slice(k, k + 16)
        for pa, pw in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):
            acc = acc + a[pa][:, s] @ w[pw][:, s].T
    return acc
