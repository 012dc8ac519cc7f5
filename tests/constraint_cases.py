"""CPU reference of constrained sampling (chemeleon_amd.Constraint, csrc/constrain.hip) and the inputs its tests
share. Test infrastructure only.

replace(): the replacement of the known entries at level s, the formulas of include/chemeleon_hip.h
(chm_constraint) op by op in torch float32, the atom types through the oracle's d3pm_q_sample.
constrained_step(): OracleModel.step restated from the oracle's own pieces (model_predictions, d3pm_p_sample, the
schedules) with stage 1 (all fields, between predictor and corrector) and stage 2 (coordinates again, behind the
corrector) interposed.
"""

import numpy as np
import torch

from chemeleon_amd import Constraint
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
from oracle import chemeleon_oracle as O

A = 104
T = 100
STEP_GATE = 1e-4  # the teacher-forced step gate on free coordinates (periodic distance) and lattices


# ------------------------------------------------------------------------------------------ the reference
def tables_of(ref):
    """{"fwd": [T+1,4] = sqrt(abar_t), sqrt(1 - abar_t), sigma_t, sigmas_norm_t, "q_mats": [T+1,A,A]} of an
    OracleModel, with the fp32 expressions Chemeleon.forward's table uses."""
    ac = ref.beta["alphas_cumprod"].float()
    fwd = torch.stack([torch.sqrt(ac), torch.sqrt(1.0 - ac), ref.sigmas.float(), ref.sigmas_norm.float()], dim=1)
    return {"fwd": fwd.contiguous(), "q_mats": ref.q_mats.float().contiguous()}


def replace(level, state, constraint, noise, tables, what=7):
    """The known entries of state = (a [N], x [N,3], l [B,3,3]) at level s; noise = (u [N,A] uniforms, z_l [B,3,3],
    z_x [N,3] normals); what: bit 0 types, bit 1 lattices, bit 2 coordinates. Returns new tensors."""
    a, x, l = (v.clone() for v in state)
    u, zl, zx = noise
    s = int(level)
    fwd = tables["fwd"]
    if what & 1 and bool(constraint.type_mask.any()):
        m = constraint.type_mask
        if s == 0:
            a[m] = constraint.atom_types[m]
        else:
            ts = torch.full((int(m.sum()),), s, dtype=torch.long)
            a[m] = O.d3pm_q_sample(constraint.atom_types[m], ts, u[m], tables["q_mats"])
    if what & 2:
        m = constraint.lattice_mask
        mask9 = O.LATTICE_MASK.float()
        v = (fwd[s, 0] * constraint.lattices + fwd[s, 1] * (zl * mask9)) * mask9
        l[m] = v[m]
    if what & 4:
        m = constraint.frac_mask
        v = (constraint.frac_coords + fwd[s, 2] * zx) % 1.0
        x[m] = v[m]
    return a, x, l


def type_score_gaps(level, constraint, u, tables):
    """float64 top-2 gap of the Gumbel scores log(q + 1e-6) - log(-log(clamp(u))) at every type-masked node."""
    m = constraint.type_mask
    q = tables["q_mats"][int(level) - 1][constraint.atom_types[m]].double()
    un = torch.clip(u[m].float(), O.EPS, 1.0).double()
    sc = torch.log(q + float(np.float32(O.EPS))) - torch.log(-torch.log(un))
    top = torch.topk(sc, 2, dim=-1).values
    return top[:, 0] - top[:, 1]


def constrained_step(ref, t, a_t, x_t, l_t, natoms, n2g, cond, null, noise, constraint, con_noise, tables,
                     cond_scale=2.0, step_lr=1e-5, stage1_late=False):
    """OracleModel.step (chemeleon.py:379-466) with the constraint interposed; the arithmetic of the unconstrained
    parts is OracleModel.step's, expression by expression. stage1_late=True is the WRONG order the tests must tell
    apart: stage 1 moved behind the corrector (its decoder call then sees the unreplaced state).
    Returns (a_{t-1}, x_{t-1}, l_{t-1})."""
    B, N = l_t.shape[0], x_t.shape[0]
    bt = torch.full((B,), t, dtype=torch.long)
    te = O.time_embedding(bt, ref.cfg["time_dim"])
    pa, pl, px = ref.model_predictions(te, a_t, x_t, l_t, natoms, n2g, cond_scale, cond, null)
    if noise is None:
        ra, rl, rx1, rx2 = torch.zeros(N, ref.A), torch.zeros(B, 3, 3), torch.zeros(N, 3), torch.zeros(N, 3)
    else:
        ra, rl, rx1, rx2 = noise
    a_prev = O.d3pm_p_sample(pa, a_t, bt[n2g], ra, ref.q_one_step, ref.q_mats)
    al, ab, sg = ref.beta["alphas"][t], ref.beta["alphas_cumprod"][t], ref.beta["sigmas"][t]
    c0 = 1.0 / torch.sqrt(al)
    c1 = (1 - al) / torch.sqrt(1 - ab)
    rl = rl * O.LATTICE_MASK
    l_prev = (c0 * (l_t - c1 * pl) + sg * rl) * O.LATTICE_MASK
    if t == ref.T:
        l_prev = l_prev.clip(-6, 6)
    sx, sn, sa = ref.sigmas[t], ref.sigmas_norm[t], ref.sigmas[t - 1]
    step = sx ** 2 - sa ** 2
    std = torch.sqrt((sa ** 2 * (sx ** 2 - sa ** 2)) / (sx ** 2))
    x_half = x_t - step * (px * torch.sqrt(sn)) + std * rx1
    if not stage1_late:  # stage 1
        a_prev, x_half, l_prev = replace(t - 1, (a_prev, x_half, l_prev), constraint, con_noise, tables, 7)
    _, _, px2 = ref.model_predictions(te, a_prev, x_half, l_prev, natoms, n2g, cond_scale, cond, null)
    step2 = step_lr * (sx / ref.sigma_begin) ** 2
    std2 = torch.sqrt(2 * step2)
    x_prev = (x_half - step2 * (px2 * torch.sqrt(sn)) + std2 * rx2) % 1.0
    if stage1_late:
        return replace(t - 1, (a_prev, x_prev, l_prev), constraint, con_noise, tables, 7)
    return replace(t - 1, (a_prev, x_prev, l_prev), constraint, con_noise, tables, 4)  # stage 2


# ------------------------------------------------------------------------------------------ Philox on the host
def philox_uniform(seed, t, kind, idx):
    """The device stream's uniforms (rng_uniform: Philox4x32-10, counter (idx lo, idx hi, t, kind), key seed;
    the first word's top 24 bits) for an array of indices; exact, as float32."""
    M = np.uint64(0xffffffff)
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1 = idx & M, idx >> np.uint64(32)
    c2 = np.full_like(idx, np.uint64(t))
    c3 = np.full_like(idx, np.uint64(kind))
    k0, k1 = np.uint64(seed) & M, np.uint64(seed) >> np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return ((c0 >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def philox_type_uniforms(seed, t, node_base, N):
    """[N, A] uniforms of stream 4 at indices (node_base + i) * 128 + class."""
    idx = (np.arange(N, dtype=np.uint64)[:, None] + np.uint64(node_base)) * np.uint64(128) + np.arange(
        A, dtype=np.uint64)[None, :]
    return torch.from_numpy(philox_uniform(seed, t, 4, idx))


# ------------------------------------------------------------------------------------------ shared inputs
def oracle_model():
    """The CPU oracle of the model tests/test_abi.py::_gpu_batch builds (synthetic weights, T = 100; the same
    seed before the constructor's Monte-Carlo sigma norms)."""
    cfg = default_config()
    cfg["timesteps"] = T
    torch.manual_seed(0)
    return O.OracleModel(cfg, synthetic_state_dict(default_config()))


def split_natoms(N):
    """Crystal sizes for N nodes: single-atom crystals included; N = 1 is one crystal (B = 1)."""
    out, k = [], 0
    sizes = (1, 2, 1, 7, 3, 40)
    while N > 0:
        n = min(N, sizes[k % len(sizes)])
        out.append(n)
        N -= n
        k += 1
    return out


KERNEL_NODES = (1, 3, 4, 5, 257)
KERNEL_MASKS = ("none", "all", "alt")
KERNEL_LEVELS = (0, 1, 50, 100)
KERNEL_SEED = 4400  # (seeds chosen so that no constrained node is a near tie: test_constraint_cases.py)
PHILOX_CASES = ((5, 100, 9, 1000, 77), (257, 50, 20, 123456789, 4321), (4, 1, 21, 3, 2), (3, 0, 21, 7, 0))
# (N, level, seed, node_base, graph_base)


def kernel_cases():
    k = 0
    for N in KERNEL_NODES:
        for mask in KERNEL_MASKS:
            for level in KERNEL_LEVELS:
                yield N, mask, level, KERNEL_SEED + k
                k += 1


def kernel_inputs(N, mask, seed):
    """(natoms, state, Constraint, noise) of a kernel-alone case. Known types include 0 and 103."""
    nat = split_natoms(N)
    B = len(nat)
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, A, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    l = torch.randn(B, 3, 3, generator=g) * 3
    a0 = torch.randint(0, A, (N,), generator=g)
    a0[0] = 103
    if N > 1:
        a0[-1] = 0
    x0 = torch.rand(N, 3, generator=g) * 3 - 1  # (outside [0, 1) too: the wrap is part of the formula)
    l0 = torch.randn(B, 3, 3, generator=g) * 3
    noise = (torch.rand(N, A, generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g))
    if mask == "none":
        nm, gm = torch.zeros(N, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)
        fm = nm.clone()
    elif mask == "all":
        nm, gm = torch.ones(N, dtype=torch.bool), torch.ones(B, dtype=torch.bool)
        fm = nm.clone()
    else:  # alternating, types and coordinates on different phases for every third node
        nm = torch.arange(N) % 2 == 0
        fm = torch.arange(N) % 3 != 1
        gm = torch.arange(B) % 2 == 1 if B > 1 else torch.ones(B, dtype=torch.bool)
    con = Constraint(nat, a0, nm, x0, fm, l0, gm)
    return nat, (a, x, l), con, noise


STEP_NATOMS = ([3, 5, 8, 1], [1])
STEP_TS = (100, 50, 2, 1)


def step_inputs(nat, t):
    """State at t, step noise, constraint and constraint noise of the whole-step tests. [3, 5, 8, 1]: types held on
    some atoms of crystals 0 and 2, the lattice of crystal 1, the coordinates of half of crystal 2. [1]: the atom's
    type and the lattice."""
    nat = list(nat)
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(7000 + 10 * t + B)
    a = torch.randint(0, A, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    l = torch.randn(B, 3, 3, generator=g) * 3 * O.LATTICE_MASK
    nz = None
    if t > 1:
        nz = (torch.rand(N, A, generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
              torch.randn(N, 3, generator=g))
    a0 = torch.randint(1, A, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.randn(B, 3, 3, generator=g) * 3 * O.LATTICE_MASK
    cnz = (torch.rand(N, A, generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g))
    tm, fm, lm = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)
    if B == 4:
        tm[[0, 2]] = True            # crystal 0: atoms 0 and 2 of 3
        tm[[8, 9, 11, 14]] = True    # crystal 2 (nodes 8..15): four of eight
        lm[1] = True
        fm[[8, 10, 12, 14]] = True   # half of crystal 2
    else:
        tm[0] = True
        lm[0] = True
    con = Constraint(nat, a0, tm, x0, fm, l0, lm)
    return (a, x, l), nz, con, cnz


def conditioning(B):
    cond, null = synthetic_text_embeds(512)
    return cond.expand(B, -1), null.expand(B, -1)
