"""CPU reference of the training forward's kernels (k_train_noise, k_train_lattice, k_train_node_loss,
k_train_reduce; csrc/kernels.hip) and the inputs their tests share. Test infrastructure only.

Two forms of one chain, on caller-given decoder outputs (types [N,A], coords [N,3], lattice [B,3,3]):
  dtype = float32: every tensor operation of OracleModel.training_forward around its decoder call (d3pm_q_sample,
    the lattice and coordinate q_sample, the score target, d3pm_q_posterior_logits twice, categorical_kl_logits,
    the cross entropy, the two MSEs and the weighted sum) as its own rounded op in the oracle's order.
    tests/test_train_cases.py pins it to the oracle bit for bit.
  dtype = float64: the same chain on the same inputs (the fp32 tables and coefficients included), widened.
The schedules are the oracle's (beta_schedule, sigma_schedule with fewer Monte-Carlo samples: the score norms are
a table the kernels read, and a noisy estimate serves as well), the D3PM tables d3pm_tables(betas, T, A), the
coefficient table [T+1][4] the one Chemeleon._train_tables writes (constraint_cases.tables_of).
"""

import functools

import torch
import torch.nn.functional as F

from chemeleon_amd.config import default_config
from oracle import chemeleon_oracle as O
from tests import constraint_cases as CC
from tests import step_cases as S

EPS32 = S.EPS32
GAP_ULPS = 32  # a node counts when its float64 top-2 gap exceeds this many fp32 ulps of its largest finite score
bits, ulps = S.bits, S.ulps

T_VALUES = (100, 1000)
CLASS_COUNTS = (5, 63, 64, 65, 104, 125)  # both sides of the 64-lane edge of the two-classes-per-lane layout
BIG = [(5 * i) % 12 + 1 for i in range(41)]  # N = 265 (not a multiple of 4), 9 B = 369: k_train_reduce's loops wrap
SHAPES = {"1": [1], "ragged": [3, 5, 8, 1], "big": BIG}
# graph g of a case runs at timesteps(T)[(g + k) % 5]: the rotations k of a shape put every timestep into it
ROTATIONS = {"1": (0, 1, 2, 3, 4), "ragged": (0, 3), "big": (0,)}
# loss weights that tell the six outputs apart (all exact in fp32)
WEIGHTS = {"d3pm_hybrid_coeff": 0.5, "cost_atom_types": 2.0, "cost_lattice": 3.0, "cost_coords": 0.25}
SIGMA_NORM_SAMPLES = 256
PLANTS = ("a0_absorbed", "xt_is_a0", "xt_absorbed", "xt_neither", "two_ones", "uniform_zero", "logits_80",
          "constant_row", "p_a0_underflows")
X0_TOP = 1.0 - 2.0 ** -24
QUANTITIES = ("target", "numerator", "kl", "ce", "loss", "vb_loss", "ce_loss", "loss_atom_types", "loss_lattice",
              "loss_coords")
OUT_NAMES = QUANTITIES[4:]


def timesteps(T):
    return (1, 2, T // 2, T - 1, T)


@functools.lru_cache(maxsize=None)
def schedules(T):
    """(beta dict, sigmas, sigmas_norm) of the oracle; the Monte-Carlo draws leave the global generator alone."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        sig, sn = O.sigma_schedule(T, sn=SIGMA_NORM_SAMPLES)
    return O.beta_schedule(T, "cosine"), sig, sn


@functools.lru_cache(maxsize=1)
def ref_model(T, A):
    """An OracleModel of T steps and A classes holding schedules and D3PM tables only (its decoder is never run: the
    tests hand it decoder outputs), with the loss weights of WEIGHTS. One at a time: the tables of T = 1000 are large."""
    m = object.__new__(O.OracleModel)
    m.cfg = dict(default_config(), timesteps=T, max_atoms=A, **WEIGHTS)
    m.T, m.A = T, A
    m.beta, m.sigmas, m.sigmas_norm = schedules(T)
    m.sigma_begin = 0.01
    m.q_one_step, m.q_mats = O.d3pm_tables(m.beta["betas"], T, A)
    m.sd = {}
    return m


def coef_table(ref):
    """[T+1][4] = {sqrt(abar), sqrt(1 - abar), sigma, sigma_norm}: the device's d_coef4."""
    return CC.tables_of(ref)["fwd"]


# ------------------------------------------------------------------------------------------ the chain
def q_scores(ref, d, dtype=torch.float32):
    """d3pm_q_sample's scores [N,A]: log(q_mats[t-1][a0] + eps) + Gumbel(clip(u, eps, 1)); argmax is x_t."""
    tn = d["t"][d["n2g"]]
    logits = torch.log(ref.q_mats[tn - 1, d["a0"], :].to(dtype) + EPS32)
    noise = torch.clip(d["ra"], EPS32, 1.0).to(dtype)
    return logits + -torch.log(-torch.log(noise))


def a_t_decisions(ref, d):
    """(class [N], counts [N] bool, exact tie [N] bool) from float64 alone. A row with two or more infinite scores
    (uniforms of exactly 1.0) is an exact tie and decides for the first of them, as torch.argmax and better() in
    kernels.hip do; any other row counts when its top-2 gap exceeds GAP_ULPS fp32 ulps of its largest finite score."""
    sc = q_scores(ref, d, torch.float64)
    cls = torch.argmax(sc, dim=-1)
    inf = torch.isinf(sc)
    tie = inf.sum(-1) >= 2
    top = torch.topk(sc, 2, dim=-1).values
    gap = (top[:, 0] - top[:, 1]).nan_to_num(0.0, posinf=float("inf"))
    mag = torch.where(inf, torch.zeros_like(sc), sc).abs().amax(-1)
    return cls, tie | (gap > GAP_ULPS * 2.0 ** -23 * mag), tie


def noised(ref, d, dtype=torch.float32):
    """The q_sample of lattices and coordinates and the score target (training_forward's lines before the decoder
    call): {"l_t", "x_t", "target", "numerator" (= d_log_p, target = numerator / sqrt(sigma_norm)), "rs" (=
    sqrt(sigma_norm) per node, float64)}."""
    t, n2g = d["t"], d["n2g"]
    ac = ref.beta["alphas_cumprod"][t]
    c0, c1 = torch.sqrt(ac).to(dtype), torch.sqrt(1.0 - ac).to(dtype)
    sig, sn = ref.sigmas[t], ref.sigmas_norm[t]
    nl = (d["nl"] * O.LATTICE_MASK).to(dtype)
    l_t = c0[:, None, None] * d["l0"].to(dtype) + c1[:, None, None] * nl
    s_a, sn_a = sig[n2g][:, None].to(dtype), sn[n2g][:, None].to(dtype)
    nx = d["nx"].to(dtype)
    num = O.d_log_p_wrapped_normal(s_a * nx, s_a)
    target = num / torch.sqrt(sn_a)
    x_t = (d["x0"].to(dtype) + s_a * nx) % 1.0
    return {"l_t": l_t, "x_t": x_t, "target": target, "numerator": num, "rs": sn[n2g].double().sqrt()}


def posterior(ref, x0, a_t, tn, x0_is_logits, dtype):
    """d3pm_q_posterior_logits."""
    x0_logits = x0.to(dtype).clone() if x0_is_logits else torch.log(F.one_hot(x0, ref.A).to(dtype) + EPS32)
    fact1 = ref.q_one_step.transpose(1, 2)[tn - 1, a_t, :].to(dtype)
    fact2 = torch.einsum("bc,bcd->bd", torch.softmax(x0_logits, dim=-1), ref.q_mats[tn - 2].to(dtype))
    out = torch.log(fact1 + EPS32) + torch.log(fact2 + EPS32)
    return torch.where((tn == 1)[:, None], x0_logits, out)


def losses(ref, d, a_t, target, dtype=torch.float32):
    """training_forward's lines behind the decoder call on d's decoder outputs, the given x_t atom types and score
    target: the six outputs by name, and the per-node "kl" and "ce" [N] whose means are vb_loss and ce_loss."""
    tn = d["t"][d["n2g"]]
    types, coords, lat = d["types"].to(dtype), d["coords"].to(dtype), d["lattice"].to(dtype)
    true_post = posterior(ref, d["a0"], a_t, tn, False, dtype)
    pred_post = posterior(ref, types, a_t, tn, True, dtype)
    l1, l2 = true_post + EPS32, pred_post + EPS32
    out = torch.softmax(l1, dim=-1) * (torch.log_softmax(l1, dim=-1) - torch.log_softmax(l2, dim=-1))
    kl = out.sum(dim=-1)
    vb = kl.mean()
    ce = F.cross_entropy(types, d["a0"])
    la = vb + ce * ref.cfg["d3pm_hybrid_coeff"]
    nl = (d["nl"] * O.LATTICE_MASK).to(dtype)
    ll = F.mse_loss(lat.masked_select(O.LATTICE_MASK), nl.masked_select(O.LATTICE_MASK))
    lx = F.mse_loss(coords, target.to(dtype))
    loss = ref.cfg["cost_atom_types"] * la + ref.cfg["cost_lattice"] * ll + ref.cfg["cost_coords"] * lx
    return {"kl": kl, "ce": F.cross_entropy(types, d["a0"], reduction="none"), "loss": loss, "vb_loss": vb,
            "ce_loss": ce, "loss_atom_types": la, "loss_lattice": ll, "loss_coords": lx}


def reference(ref, d, dtype):
    """The whole chain in one dtype: noised() and losses() on the float64 decisions' x_t (which the float32
    q_sample shares wherever every node counts)."""
    a_t = a_t_decisions(ref, d)[0]
    r = noised(ref, d, dtype)
    r.update(losses(ref, d, a_t, r["target"], dtype))
    r["a_t"] = a_t
    return r


# ------------------------------------------------------------------------------------------ errors
def scaled(got, want, floor=0.0):
    """Largest |got - want| / max(|want|, rms(want), floor); floor = 0 is what tests/test_gpu_train.py measures."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    if want.numel() == 0:
        return 0.0
    scale = max(float(want.pow(2).mean().sqrt()), 1e-12, floor)
    return float(((got - want).abs() / torch.maximum(want.abs(), torch.full_like(want, scale))).max())


# The KL of a node is a sum of p (log p - log q) over log-probabilities as large as -log(1e-6) = 13.8 and cancels to
# ~1e-6 where the two posteriors agree (t near T, and one-node batches have no other node to set the scale): its
# error, and that of the outputs it enters, is taken relative to max(|value|, 1), one unit of those log-probabilities.
FLOORS = {"kl": 1.0, "vb_loss": 1.0, "loss_atom_types": 1.0, "loss": 1.0}


def errors(got, r64, d):
    """Per quantity of QUANTITIES the error of `got` (device results or the float32 restatement: target [N,3], kl,
    ce [N] and the six outputs by name) against the float64 chain r64 on the inputs d. The score target as
    test_gpu_train.py compares it: nodes with sqrt(sigma_norm) >= 1e-2 directly, the others through the numerator
    target * sqrt(sigma_norm). Near t = T that target is float32 rounding noise divided by sqrt(sigma_norm) ~ 1e-8,
    values of order 1 that no two float32 evaluations share; so, again as test_gpu_train.py, loss_coords and its
    share of loss are held against the float64 MSE over got's OWN target, which the two lines above have checked."""
    rs = r64["rs"]
    good = rs >= 1e-2
    tg, t64 = got["target"].double(), r64["target"]
    e = {"target": scaled(tg[good], t64[good]),
         "numerator": float(((tg - t64) * rs[:, None])[~good].abs().max()) if bool((~good).any()) else 0.0,
         "kl": scaled(got["kl"], r64["kl"], FLOORS["kl"]), "ce": scaled(got["ce"], r64["ce"])}
    lx = ((d["coords"].double() - tg) ** 2).mean()
    want = dict(r64, loss_coords=lx, loss=r64["loss"] + WEIGHTS["cost_coords"] * (lx - r64["loss_coords"]))
    for k in OUT_NAMES:
        e[k] = scaled(got[k].reshape(1), want[k].reshape(1), FLOORS.get(k, 0.0))
    return e


# ------------------------------------------------------------------------------------------ inputs
SEED0 = 31000
SEEDS = {}  # (shape name, T, A, k) -> seed, where SEED0's did not make every node count


def cases():
    """(shape name, natoms, T, A) of the kernel tests; each runs at the rotations ROTATIONS[name]."""
    for T in T_VALUES:
        for A in CLASS_COUNTS:
            for name, nat in SHAPES.items():
                yield name, nat, T, A


def seed_of(name, T, A, k):
    return SEEDS.get((name, T, A, k), SEED0 + 1000 * list(SHAPES).index(name) + 100 * T_VALUES.index(T) + 10 * CLASS_COUNTS.index(A) + k)


def inputs(name, T, A, k):
    """One case's inputs, every edge planted. Returns a dict of CPU tensors:
      nat, n2g, t [B]                  the crystals and their timesteps, timesteps(T)[(g + k) % 5]
      a0 [N], x0 [N,3], l0 [B,3,3]     the clean state
      ra [N,A], nl [B,3,3], nx [N,3]   the draws (nl unmasked, as training_forward takes it)
      types, coords, lattice           the decoder outputs
      plants                           {plant name: node} of what was planted
    Node j < 9 holds plant PLANTS[(j + salt) % 9], salt = k + the class count's index + 3 * T's index: a batch of 9
    nodes or more holds every plant, and the one-atom batch holds each over its cases. Node 0's coordinates are
    x0 = 0 with negative noise (wraps from below), x0 = 1 - 2^-24, and x0 = 0.999 with noise +3 (wraps from above)."""
    nat = SHAPES[name]
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(seed_of(name, T, A, k))
    ts = timesteps(T)
    d = {"nat": torch.tensor(nat), "n2g": torch.arange(B).repeat_interleave(torch.tensor(nat)),
         "t": torch.tensor([ts[(i + k) % 5] for i in range(B)], dtype=torch.long)}
    a0 = torch.randint(1, A, (N,), generator=g)
    a0[torch.rand(N, generator=g) < 0.25] = 0
    d["a0"] = a0
    d["x0"] = torch.rand(N, 3, generator=g)
    d["l0"] = torch.randn(B, 3, 3, generator=g) * 3
    d["ra"] = torch.rand(N, A, generator=g)
    d["nl"] = torch.randn(B, 3, 3, generator=g)
    d["nx"] = torch.randn(N, 3, generator=g)
    d["types"] = torch.randn(N, A, generator=g) * 2
    d["coords"] = torch.randn(N, 3, generator=g)
    d["lattice"] = torch.randn(B, 3, 3, generator=g)
    d["x0"][0] = torch.tensor([0.0, X0_TOP, 0.999])
    d["nx"][0, 0], d["nx"][0, 2] = -0.75, 3.0
    salt = k + CLASS_COUNTS.index(A) + 3 * T_VALUES.index(T)
    d["plants"] = {}
    for j in range(min(N, len(PLANTS))):
        p = PLANTS[(j + salt) % len(PLANTS)]
        d["plants"][p] = j
        c = 1 + j % (A - 1)  # a class that is not the absorbing one
        if p == "a0_absorbed":
            a0[j] = 0
        elif p == "xt_is_a0":
            a0[j] = c
            d["ra"][j, c] = 1.0
        elif p == "xt_absorbed":
            a0[j] = c
            d["ra"][j, 0] = 1.0
        elif p == "xt_neither":
            a0[j] = c
            d["ra"][j, c + 1 if c + 1 < A else c - 1] = 1.0
        elif p == "two_ones":
            d["ra"][j, 1] = d["ra"][j, A - 1] = 1.0
        elif p == "uniform_zero":
            d["ra"][j, int(a0[j])] = 0.0
        elif p == "logits_80":
            d["types"][j, 0::2], d["types"][j, 1::2] = 80.0, -80.0
        elif p == "constant_row":
            d["types"][j] = 1.25
        elif p == "p_a0_underflows":
            d["types"][j, int(a0[j])] = -110.0
            d["types"][j, (int(a0[j]) + 1) % A] = 20.0
    return d
