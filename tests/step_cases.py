"""CPU reference of the reverse step's update kernels (k_step_predictor, k_d3pm as the step calls it,
k_step_corrector; csrc/kernels.hip) and the inputs their tests share. Test infrastructure only.

Two forms of one chain, on caller-given decoder outputs (types [2,N,A], coords [2,N,3], lattice [2,B,3,3], the
conditional outputs first, then the null ones):
  dtype = float32: every tensor operation of OracleModel.model_predictions / step / d3pm_p_sample as its own
    rounded op in the oracle's order: the mix (w_null n) + (w_cond c), (c0 (l - c1 pl) + sg (z mask)) mask, the
    clip at t == T, x - step (px sqrt_sn) + std z, % 1.0. tests/test_step_cases.py pins it to the oracle bit for bit.
  dtype = float64: the same chain on the same inputs (coefficients and weights included), widened.
The coefficients come from coef_table(), the [T+1][8] table the device reads (Chemeleon.schedule_tables; the GPU
tests require the model's table to equal it bit for bit). The guidance weights are weights(): the two floats the
ABI forms from a float cond_scale, or the reference's.
"""

import numpy as np
import torch

from oracle import chemeleon_oracle as O
from tests import constraint_cases as CC

A, T = CC.A, CC.T
STEP_LR = 1e-5
EPS32 = float(np.float32(O.EPS))
GAP_ULPS = 32  # a node counts when its float64 top-2 gap exceeds this many fp32 ulps of its largest score magnitude

oracle_model = CC.oracle_model
philox_uniform = CC.philox_uniform

SHAPES = {
    "1": [1],                 # the smallest batch
    "ragged": [3, 5, 8, 1],   # a small ragged batch
    "85": [85],               # 3N = 255: the nine lattice elements straddle k_step_predictor's first block
    "43x2": [43, 43],         # N = 86, 3N = 258
    "1x29": [1] * 29,         # B 9 = 261 lattice elements against 87 coordinates
}
BIG = [1] * 16389             # more than 4096 * 4 nodes: k_d3pm's grid-stride loop runs a second pass
TS = (100, 99, 50, 2, 1)
COND_SCALES = (2.0, 1.0, 0.0, 1.3)
SCALE_TS = (100, 50, 1)       # the cond_scale cases run on the ragged batch at these t
D3PM_A = (1, 63, 64, 65, 104, 128)
D3PM_N = (1, 4, 5)
NAN_CLASS = 17                # at t = 1 one node's conditional logit of this class is NaN
# corrector inputs whose unwrapped result is exactly: 0, -0.0, 1.0, above 1, below -1, a tiny negative (% 1.0 -> 1.0)
WRAP_EDGES = (0.0, -0.0, 1.0, 1.75, -1.25, -1.0e-9)


def coef_table(ref, step_lr=STEP_LR):
    """[T+1][8] = {c0, c1, sigma_l, step_x, std_x, sqrt(sigma_norm), step2, std2}: OracleModel.step's scalar
    expressions (chemeleon.py:413-457) per t, as Chemeleon.schedule_tables writes the device table."""
    coef = torch.zeros(ref.T + 1, 8)
    for t in range(1, ref.T + 1):
        al, ab, sg = ref.beta["alphas"][t], ref.beta["alphas_cumprod"][t], ref.beta["sigmas"][t]
        c0 = 1.0 / torch.sqrt(al)
        c1 = (1 - al) / torch.sqrt(1 - ab)
        sx, sn, sa = ref.sigmas[t], ref.sigmas_norm[t], ref.sigmas[t - 1]
        step = sx ** 2 - sa ** 2
        std = torch.sqrt((sa ** 2 * (sx ** 2 - sa ** 2)) / (sx ** 2))
        step2 = step_lr * (sx / ref.sigma_begin) ** 2
        std2 = torch.sqrt(2 * step2)
        coef[t] = torch.stack([c0, c1, sg, step, std, torch.sqrt(sn), step2, std2])
    return coef


def weights(cond_scale, abi=True):
    """(w_null, w_cond) as Python floats holding fp32 values. abi: what sample_step forms from the ABI's float
    cond_scale, (float)(1.0 - (double)cs32); else the reference's: 1 - cond_scale in double from the Python
    float, rounded once when it meets the float32 tensor. Equal wherever cond_scale is itself a float."""
    cs32 = np.float32(cond_scale)
    w_null = np.float32(1.0 - float(cs32)) if abi else np.float32(1.0 - float(cond_scale))
    return float(w_null), float(cs32)


def mix(pair, w, dtype=torch.float32):
    """model_predictions' (1 - cond_scale) * null + cond_scale * cond on pair = [cond, null]."""
    p = pair.to(dtype)
    return (w[0] * p[1]) + (w[1] * p[0])


def predictor(t, x, l, coords, lattice, rl, rx1, coef, w, dtype=torch.float32, T_=T, clip=True):
    """(x_half, l_prev): the VE predictor half step and the DDPM lattice update; rl / rx1 None = zero noise."""
    cf = coef[t].to(dtype)
    mask = O.LATTICE_MASK.to(dtype)
    x, l = x.to(dtype), l.to(dtype)
    zl = torch.zeros_like(l) if rl is None else rl.to(dtype)
    zx = torch.zeros_like(x) if rx1 is None else rx1.to(dtype)
    pl, px = mix(lattice, w, dtype), mix(coords, w, dtype)
    l_prev = (cf[0] * (l - cf[1] * pl) + cf[2] * (zl * mask)) * mask
    if clip and t == T_:
        l_prev = l_prev.clip(-6, 6)
    x_half = x - cf[3] * (px * cf[5]) + cf[4] * zx
    return x_half, l_prev


def corrector(t, x, coords, rx2, coef, w, dtype=torch.float32, wrap=True):
    """The Langevin move and the wrap to [0, 1); rx2 None = zero noise. wrap=False: the unwrapped value."""
    cf = coef[t].to(dtype)
    x = x.to(dtype)
    zx = torch.zeros_like(x) if rx2 is None else rx2.to(dtype)
    xn = x - cf[6] * (mix(coords, w, dtype) * cf[5]) + cf[7] * zx
    return xn % 1.0 if wrap else xn


def types32(t_node, a, types, ra, q1, qm, w):
    """The oracle's d3pm_p_sample on the float32 mix; ra None = the zeros OracleModel.step passes at t == 1."""
    ra = torch.zeros(types.shape[1:]) if ra is None else ra
    return O.d3pm_p_sample(mix(types, w), a, t_node, ra, q1, qm)


def scores64(t_node, a, logits, ra, q1, qm):
    """float64 D3PM scores [N,A] on float64 logits: posterior + Gumbel where t > 1, the logits at t == 1
    (d3pm_p_sample widened; eps is the float32 1e-6 both sides add)."""
    q1, qm = q1.double(), qm.double()
    N, A_ = logits.shape
    sm = torch.softmax(logits, dim=-1)
    fact1 = q1.transpose(1, 2)[t_node - 1, a, :]
    fact2 = torch.empty(N, A_, dtype=torch.float64)
    for tv in torch.unique(t_node).tolist():  # (per t one matmul: no [N,A,A] gather)
        m = t_node == tv
        fact2[m] = sm[m] @ qm[tv - 2]
    out = torch.log(fact1 + EPS32) + torch.log(fact2 + EPS32)
    first = (t_node == 1)[:, None]
    post = torch.where(first, logits, out)
    ra = torch.zeros(N, A_) if ra is None else ra
    g = -torch.log(-torch.log(torch.clamp(ra.float(), min=EPS32, max=1.0).double()))
    return post + g * (~first).double()


def type_decisions(t_node, a, types, ra, q1, qm, w):
    """(class [N], counts [N] bool, gap [N], threshold [N]) from float64 alone. types [2,N,A] are mixed in float64
    with weights w, or [N,A] logits taken as they are (w None). A node counts when its top-2 gap exceeds GAP_ULPS
    fp32 ulps of its largest score magnitude (at t == 1 the two products of the mix count as scores: the sum may
    cancel). A row with a NaN decides for its first NaN (torch.argmax, and better() in kernels.hip) and counts."""
    if w is None:
        logits, mag0 = types.double(), torch.zeros(types.shape[0], dtype=torch.float64)
    else:
        p = types.double()
        logits = (w[0] * p[1]) + (w[1] * p[0])
        mag0 = torch.maximum((w[0] * p[1]).abs(), (w[1] * p[0]).abs()).nan_to_num(0.0).amax(-1)
        mag0 = torch.where(t_node == 1, mag0, torch.zeros_like(mag0))
    sc = scores64(t_node, a, logits, ra, q1, qm)
    nan_row = sc.isnan().any(-1)
    cls = torch.argmax(sc, dim=-1)
    s0 = sc.nan_to_num(float("-inf"))
    if sc.shape[1] > 1:
        top = torch.topk(s0, 2, dim=-1).values
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full((sc.shape[0],), float("inf"), dtype=torch.float64)
    gap = torch.where(nan_row, torch.full_like(gap, float("inf")), gap)
    mag = torch.maximum(sc.nan_to_num(0.0, 0.0, 0.0).abs().amax(-1), mag0)
    thr = GAP_ULPS * 2.0 ** -23 * mag
    return cls, gap > thr, gap, thr


# ------------------------------------------------------------------------------------------ inputs
SEED0 = 9100
SEEDS = {("big", 100): 14103}  # (shape name, t) -> seed, where SEED0's did not make every node count


def cases():
    """(shape name, natoms, t) of the update tests at cond_scale 2.0, the large batch included."""
    for name, nat in list(SHAPES.items()) + [("big", BIG)]:
        for t in TS:
            yield name, nat, t


def seed_of(name, t):
    """Seeds chosen so that every node of every case counts (tests/test_step_cases.py asserts it). t = T - 1 takes
    t = T's seed: the same inputs, which clip at T, must not clip at T - 1."""
    t = T if t == T - 1 else t
    k = list(SHAPES).index(name) if name in SHAPES else len(SHAPES)
    return SEEDS.get((name, t), SEED0 + 1000 * k + t)


def inputs(nat, t, seed, coef, w=None):
    """One case's inputs, every edge planted. Returns a dict of CPU tensors:
      a [N], x [N,3], l [B,3,3]          the state before the predictor (l unmasked: the masked entries are non-zero)
      types, coords, lattice             the predictor's decoder outputs [2,...]
      x2 [N,3], coords2 [2,N,3]          the corrector's state and decoder outputs
      ra, rl, rx1, rx2                   the four noise tensors (used at t == 1 only where a test says so)
      wrap_edges                         the WRAP_EDGES planted in x2 (flat entries 0..)
    Planted: graph 0's lattice holds entries that the t == T clip cuts at +6 and at -6 and one it leaves alone (the
    inputs of t = T - 1 are those of t = T);
    x_t = 0 and A - 1; at t == 1 a NaN logit; the corrector's wrap edges (their coords2 rows are 0, their noise -0.0,
    so the unwrapped value is x2 itself)."""
    w = weights(2.0) if w is None else w
    B, N = len(nat), sum(nat)
    tp = T if t == T - 1 else t  # (what is planted at T - 1 is what is planted at T)
    g = torch.Generator().manual_seed(seed)
    d = {}
    a = torch.randint(0, A, (N,), generator=g)
    a[torch.rand(N, generator=g) < 0.5] = 0      # the absorbed class, the state every node starts from
    a[0] = 0 if (N > 1 or tp % 2 == 0) else A - 1
    if N > 1:
        a[-1] = A - 1
    d["a"] = a
    d["x"] = torch.rand(N, 3, generator=g)
    d["l"] = torch.randn(B, 3, 3, generator=g) * 3
    d["types"] = torch.randn(2, N, A, generator=g) * 2
    d["coords"] = torch.randn(2, N, 3, generator=g)
    d["lattice"] = torch.randn(2, B, 3, 3, generator=g)
    d["ra"] = torch.rand(N, A, generator=g)
    d["rl"] = torch.randn(B, 3, 3, generator=g)
    d["rx1"] = torch.randn(N, 3, generator=g)
    d["rx2"] = torch.randn(N, 3, generator=g)
    d["x2"] = torch.rand(N, 3, generator=g) * 2 - 0.5
    d["coords2"] = torch.randn(2, N, 3, generator=g)
    # the clip: +-40 leave [-6, 6] at T (c0 = 100) and at T - 1; c1 pl itself lands near the noise term, inside
    cf = coef[tp]
    d["l"][0, 0, 0], d["l"][0, 1, 1] = 40.0, -40.0
    d["l"][0, 2, 2] = cf[1] * mix(d["lattice"], w)[0, 2, 2]
    if t == 1:
        d["types"][0, N // 2, NAN_CLASS] = float("nan")
    k0 = 0 if 3 * N >= len(WRAP_EDGES) else 3 * (tp % 2)
    edges = WRAP_EDGES[k0:k0 + min(3 * N, len(WRAP_EDGES))]
    x2, c2, z2 = d["x2"].view(-1), d["coords2"].view(2, -1), d["rx2"].view(-1)
    for k, v in enumerate(edges):
        x2[k] = v
        c2[:, k] = 0.0
        z2[k] = -0.0
    d["wrap_edges"] = edges
    return d


def d3pm_inputs(A_, N, seed):
    """chm_d3pm_sample's own case: logits [N,A], x_t with 0 and A - 1, per-node t covering 1, 2 and T, noise."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(N, A_, generator=g) * 2
    xt = torch.randint(0, A_, (N,), generator=g)
    xt[0] = 0
    xt[-1] = A_ - 1 if N > 1 else xt[-1]
    tn = torch.tensor([(1, 2, T, 50, T - 1)[(i + A_ + N) % 5] for i in range(N)], dtype=torch.long)
    if N >= 4:
        tn[:3] = torch.tensor([1, 2, T])
    u = torch.rand(N, A_, generator=g)
    return lg, xt, tn, u


def d3pm_tables(ref, A_):
    return O.d3pm_tables(ref.beta["betas"], ref.T, A_)


def d3pm_seed(A_, N):
    return 5000 + 10 * A_ + N


def bits(t):
    """The bit patterns of a float32 tensor, so that -0.0 != 0.0 and NaN == NaN."""
    return t.contiguous().view(torch.int32)


def ulps(got, want):
    """Per element, the distance in fp32 ulps between two finite float32 tensors (-0.0 and 0.0 are 1 apart)."""
    def key(v):
        i = bits(v).long()
        return torch.where(i < 0, -(i & 0x7fffffff) - 1, i)
    return (key(got) - key(want)).abs()
