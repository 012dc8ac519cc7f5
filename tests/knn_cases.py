"""Cases and an independent reference of the radius-graph ("knn") edge path (csrc/knn.hip, knn_build in
csrc/decoder.hip, the node-aligned segment tiles of edge layer 2), for tests/test_knn_cases.py on the CPU and
tests/test_gpu_knn_kernels.py on the GPU. A plain helper module: every input is seeded or exact.

The reference (`graph`) is written from the definition in numpy float64 and Python integers; it shares no code
with oracle/knn_oracle.py (the torch fp32 restatement of the reference repository), and the CPU test holds the two
against each other. Per crystal, for every candidate (atom1 i, atom2 j, cell c) of the 27 neighbouring cells:

    d2 = |pos_i - (pos_j + u_c L)|^2,  pos = frac L,  u_c in {-1, 0, 1}^3 with the last axis fastest
    radius:  kept when 1e-4 < d2 <= r^2,  r = the smallest interplanar spacing + 0.01
    cap:     an atom with more than max_nb kept candidates (max_nb > 0) keeps d2 < v + 0.01, v its (max_nb+1)-th
             smallest d2; otherwise all
    one direction: j < i, or j == i with an "earlier" cell (the first non-zero component of u negative); the edge
             is (src, dst) = (j, i) with frac_diff = -(x_j - x_i + u), followed, after all of the crystal's kept
             edges, by the reverses (i, j) with +(x_j - x_i + u)
    final:   the batch's edges grouped by source node, each node's in list order (a stable sort by source)

frac_diff is part of the definition and is computed in float32 as the kernel rounds it: fl(fl(x_j - x_i) + u).

Every decision carries a margin, the relative distance of d2 from the cut that decided it. The cases are chosen so
that no margin is below 1e-4 (test_knn_cases.py asserts it) while fp32 rounding moves d2, r^2 and v + 0.01 by less
than 1e-6: the device and this reference cannot legitimately disagree on any of them, so the GPU tests compare
graphs exactly.

The exact crystals have coordinates on the 1/16 grid and lattices of small integers or powers of two: every product
and sum of the kernel's fp32 expression for d2 is then exact and ties are exact ties (`d2_fp32` restates that
expression for the check). Degrees and candidate counts of the simple-cubic supercells follow from the number of
integer vectors with |v|^2 <= 16, which is 257: the 4x4x4 supercell with a = 4 has exactly 256 candidates per atom
(uncapped: degree 256, the supported maximum); scaled to a = 1/4 the + 0.01 of the radius takes in the 48 vectors of
|v|^2 = 17 as well (304 candidates per atom: the refusal above 256 edges)."""

import functools

import numpy as np

from tests import edge_cases as EC

H, NF = EC.H, EC.NF
MARGIN = 1e-4
MAX_DEG = 256          # edges per node (a segment tile's rows)
MAX_ATOMS = 256        # atoms per crystal
PER_ATOM = 128         # the default edge capacity per atom (chm_batch_options.knn_edges_per_atom)

# u of cell c (last axis fastest) and the cells "earlier" than their mirror 26 - c
CELLS = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.int64)
EARLIER = np.array([tuple(u) < (0, 0, 0) for u in CELLS.tolist()])  # lexicographic: first non-zero component < 0

EDGELESS_LATTICE = [[4, 0, 0], [4, 4, 0], [0, 4, 4]]  # spacings 2.31, 2.83, 4; shortest lattice vector 4


# ---------------------------------------------------------------- the reference

def radius2(L):
    """r^2 of one crystal, float64: (smallest interplanar spacing + 0.01)^2."""
    L = np.asarray(L, np.float64)
    vol = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
    sp = [vol / float(np.linalg.norm(np.cross(L[(k + 1) % 3], L[(k + 2) % 3]))) for k in range(3)]
    r = min(sp) + 0.01
    return r * r


def _d2(x, L):
    """d2 [n, n, 27] float64 of one crystal."""
    pos = x @ L
    off = CELLS.astype(np.float64) @ L
    d = pos[:, None, None, :] - (pos[None, :, None, :] + off[None, None, :, :])
    return (d * d).sum(-1)


def d2_fp32(x, L):
    """d2 [n, n, 27] as k_knn_pairs' fp32 expression gives it (every operation rounded on its own, in its order)."""
    x, L = np.asarray(x, np.float32), np.asarray(L, np.float32)
    f = np.float32
    pos = ((x[:, 0:1] * L[0][None, :]).astype(f) + (x[:, 1:2] * L[1][None, :]).astype(f)).astype(f)
    pos = (pos + (x[:, 2:3] * L[2][None, :]).astype(f)).astype(f)
    u = CELLS.astype(f)
    off = ((u[:, 0:1] * L[0][None, :]).astype(f) + (u[:, 1:2] * L[1][None, :]).astype(f)).astype(f)
    off = (off + (u[:, 2:3] * L[2][None, :]).astype(f)).astype(f)
    d = (pos[:, None, None, :] - (pos[None, :, None, :] + off[None, None, :, :]).astype(f)).astype(f)
    q = (d * d).astype(f)
    return ((q[..., 0] + q[..., 1]).astype(f) + q[..., 2]).astype(f)


def crystal(x32, L32, max_nb):
    """The decisions of one crystal. x32 [n, 3], L32 [3, 3] float32 inputs (taken to float64 exactly).
    Returns a dict: d2 [n, n, 27]; in_radius, kept [n, n, 27] bool (after the radius / after the cap);
    ncand, nkept [n]; cut [n] (inf for an atom the cap leaves alone); radius_margin, cap_margin (the smallest relative
    margins, inf when nothing was decided); tie_at_cap [n] bool (the max_nb-th and (max_nb+1)-th smallest are equal);
    one_sided (kept candidates whose mirror candidate is not kept); directed [D, 3] (i, j, c) in list order."""
    x, L = np.asarray(x32, np.float64), np.asarray(L32, np.float64)
    n = len(x)
    d2 = _d2(x, L)
    r2 = radius2(L)
    inr = (d2 > 1e-4) & (d2 <= r2)
    rm = float(min((np.abs(d2 - r2) / r2).min(), (np.abs(d2 - 1e-4) / 1e-4).min()))
    kept = inr.copy()
    cut = np.full(n, np.inf)
    tie = np.zeros(n, bool)
    cm = np.inf
    ncand = inr.reshape(n, -1).sum(1)
    for i in range(n):
        c = int(ncand[i])
        if max_nb > 0 and c > max_nb:
            mine = np.sort(d2[i][inr[i]])
            v = float(mine[max_nb])
            cut[i] = v + 0.01
            tie[i] = mine[max_nb - 1] == mine[max_nb]
            cm = min(cm, float((np.abs(mine - cut[i]) / cut[i]).min()))
            kept[i] &= d2[i] < cut[i]
    mirror = kept.transpose(1, 0, 2)[:, :, ::-1]  # candidate (j, i, 26 - c)
    ii, jj, cc = np.nonzero(kept)                 # list order: atom1 major, atom2, cell fastest
    one_dir = (jj < ii) | ((jj == ii) & EARLIER[cc])
    return dict(d2=d2, in_radius=inr, kept=kept, ncand=ncand, nkept=kept.reshape(n, -1).sum(1), cut=cut,
                radius_margin=rm, cap_margin=float(cm), tie_at_cap=tie, one_sided=int((kept & ~mirror).sum()),
                directed=np.stack([ii[one_dir], jj[one_dir], cc[one_dir]], 1))


def graph(natoms, frac, lattices, max_nb):
    """The reference graph of a batch. Returns a dict: src, dst [E] int64 (global node indices, grouped by source, list
    order within a node), fd [E, 3] float32, deg [N] (out-degrees), E, per-crystal decision dicts `crystals`, and the
    batch's smallest margins."""
    frac = np.asarray(frac, np.float32)
    lattices = np.asarray(lattices, np.float32)
    src, dst, fd, cr = [], [], [], []
    off = 0
    for b, n in enumerate(natoms):
        x = frac[off:off + n]
        c = crystal(x, lattices[b], max_nb)
        cr.append(c)
        i, j, cell = c["directed"].T
        ev = ((x[j] - x[i]).astype(np.float32) + CELLS[cell].astype(np.float32)).astype(np.float32)
        src += [j + off, i + off]  # the kept direction (atom2 -> atom1), then the reverses
        dst += [i + off, j + off]
        fd += [-ev, ev]
        off += n
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    fd = np.concatenate(fd).astype(np.float32).reshape(-1, 3)
    order = np.argsort(src, kind="stable")
    src, dst, fd = src[order], dst[order], fd[order]
    return dict(src=src, dst=dst, fd=fd, deg=np.bincount(src, minlength=off), E=len(src), crystals=cr,
                radius_margin=min(c["radius_margin"] for c in cr), cap_margin=min(c["cap_margin"] for c in cr))


# ---------------------------------------------------------------- crystals

def _diag(a, b=None, c=None):
    return [[a, 0, 0], [0, a if b is None else b, 0], [0, 0, a if c is None else c]]


def grid_crystal(dims, n=None, spacing=1.0, seed=None):
    """n atoms (default all) on the sites of a dims[0] x dims[1] x dims[2] simple-cubic grid in the cell
    diag(dims) spacing; seed: the sites in a seeded random order (atom indices then say nothing about positions, and
    n below the site count leaves vacancies), else row-major. dims in {1, 2, 4, 8, 16}: exact fp32."""
    sites = np.array([[a, b, c] for a in range(dims[0]) for b in range(dims[1]) for c in range(dims[2])], np.float64)
    if seed is not None:
        sites = sites[np.random.default_rng([seed, *dims]).permutation(len(sites))]
    sites = sites[:len(sites) if n is None else n]
    x = (sites / np.asarray(dims, np.float64)).astype(np.float32)
    L = (np.diag(np.asarray(dims, np.float64)) * spacing).astype(np.float32)
    return x, L


def _cubic(basis, a=4.0):
    return np.asarray(basis, np.float32), np.asarray(_diag(a), np.float32)


SC1 = _cubic([[3 / 16, 5 / 16, 1 / 2]])
BCC = _cubic([[0, 0, 0], [.5, .5, .5]])
FCC = _cubic([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
DIAMOND = _cubic([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0],
                  [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])
# distinct atoms on the 1/16 grid in a sheared dyadic cell: every neighbourhood differs
DYADIC = (np.asarray([[1, 2, 3], [9, 4, 14], [5, 11, 7], [12, 13, 2], [15, 6, 10], [3, 8, 8], [10, 1, 5]], np.float32) / 16,
          np.asarray([[4, 0, 0], [1, 4, 0], [.5, 1, 2]], np.float32))
EDGELESS = (np.asarray([[1 / 4, 1 / 2, 3 / 4]], np.float32), np.asarray(EDGELESS_LATTICE, np.float32))
# two atoms 1 apart in the sheared cell: one edge each way and no image within the radius (degree 1 and 1)
PAIR = (np.asarray([[0, 0, 0], [1 / 4, 0, 0]], np.float32), np.asarray(EDGELESS_LATTICE, np.float32))


def _cluster():
    """A 3 x 3 x 3 block of atoms with spacing 1 in the cell 16 I (r = 16.01) and one atom 9 away from it, in the
    middle of the index range: the distant atom's cap keeps pairs that the block atoms' caps drop."""
    blk = [[a, b, c] for a in range(3) for b in range(3) for c in range(3)]
    sites = blk[:13] + [[11, 1, 1]] + blk[13:]
    return np.asarray(sites, np.float32) / 16, np.asarray(_diag(16.0), np.float32)


CLUSTER = _cluster()


def plate(n, seed, ratio):
    """n atoms at generic coordinates slightly outside [0, 1) (as the corrector's unwrapped ones) in a sheared cell
    whose third axis is `ratio` times shorter than the others: the radius follows the short axis, so an atom has
    O(n ratio^2) candidates instead of 4 n and a seed without an undecided decision exists."""
    rng = np.random.default_rng([seed, n])
    x = (rng.random((n, 3)) * 1.2 - 0.1).astype(np.float32)
    a = (14.0 * n * ratio) ** (1 / 3)  # about 15 cubic Angstrom per atom
    L = np.diag([a, a * 1.1, a / ratio]) + 0.05 * a / ratio * (rng.random((3, 3)) - 0.5)
    return x, L.astype(np.float32)


def _batch(*crystals):
    return ([len(c[0]) for c in crystals], np.concatenate([c[0] for c in crystals]).astype(np.float32),
            np.stack([c[1] for c in crystals]).astype(np.float32))


SC64 = grid_crystal((4, 4, 4), seed=1)
SC64_FINE = grid_crystal((4, 4, 4), spacing=1 / 16, seed=1)
SC256 = grid_crystal((8, 8, 4), seed=2)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (natoms, frac [N, 3] f32, lattices [B, 3, 3] f32, max_nb, knn_edges_per_atom). Read-only arrays."""
    c = {}

    def add(name, crystals, max_nb=20, per_atom=PER_ATOM):
        nat, x, L = _batch(*crystals)
        x.setflags(write=False)
        L.setflags(write=False)
        c[name] = (nat, x, L, max_nb, per_atom)

    # exact crystals
    add("sc1", [SC1])
    add("bcc", [BCC])
    add("bcc_cap6", [BCC], 6)          # 8 + 6 candidates, the cap inside the shell of 8: degree 8
    add("fcc", [FCC])
    add("diamond", [DIAMOND])          # 4, 12, 12, 6: the 21st inside the second shell of 12
    add("sc64", [SC64])                # 6, 12, 8, ...: the 21st inside the shell of 8; 256 candidates per atom
    add("sc64_fine", [SC64_FINE])      # a = 1/4: 304 candidates per atom
    add("sc256", [SC256])              # 8 x 8 x 4: atom index 255 in both key bytes
    add("dyadic", [DYADIC])
    # sizes (grid crystals with vacancies, seeded site order), alone and ragged
    for n, dims in ((1, (1, 1, 1)), (2, (2, 1, 1)), (5, (2, 2, 2)), (63, (4, 4, 4)), (65, (8, 4, 4)), (255, (8, 8, 4))):
        add(f"n{n}", [grid_crystal(dims, n, seed=10 + n)])
    add("ragged_1_between", [grid_crystal((8, 8, 4), 255, seed=265), SC1, SC256])
    add("ragged_small", [grid_crystal((2, 2, 2), 5, seed=15), grid_crystal((4, 4, 4), 63, seed=73), BCC, SC64,
                         grid_crystal((8, 4, 4), 65, seed=75), SC1, grid_crystal((2, 1, 1), 2, seed=12)])
    # the cap
    for m in (1, 6, 12, 18):
        add(f"sc64_cap{m}", [SC64], m)
    for m in (0, -1, 256, 300):        # uncapped, and a cap no atom reaches: degree 256, the supported maximum
        add(f"sc64_cap{m}", [SC64], m, 256)
    add("fcc_cap18", [FCC], 18)        # 18 candidates: c == max_nb
    add("fcc_cap17", [FCC], 17)        # c == max_nb + 1
    add("n63_cap252", [grid_crystal((4, 4, 4), 63, seed=73)], 252, 256)  # both in one crystal (vacancy neighbours)
    add("cluster", [CLUSTER])          # one-sided pairs
    # atoms without edges
    add("edgeless1", [EDGELESS])
    add("edgeless_batch", [EDGELESS] * 7)
    add("mixed_edgeless", [FCC, EDGELESS, BCC] + [EDGELESS] * 300 + [DIAMOND, EDGELESS, PAIR, SC1])
    add("edgeless_run600", [BCC] + [EDGELESS] * 600 + [FCC])  # a whole segment tile of 256 nodes without a row
    # degrees 248-255 (every node a tile of its own) next to nodes of degree 1 and 0
    add("hub_and_leaves", [PAIR] * 3 + [grid_crystal((4, 4, 4), 63, seed=73)] + [PAIR] * 40 + [EDGELESS] * 2 + [PAIR],
        0, 256)
    # generic coordinates
    add("random_small", [plate(n, 3, 1.0) for n in (1, 2, 3, 5)] + [plate(7, 3, 1.5), plate(12, 4, 2.0)])
    add("random_mid", [plate(30, 1, 3.0), plate(64, 1, 5.0), plate(17, 2, 2.5)])
    add("random_256", [plate(256, 6, 9.0), plate(1, 5, 1.0), plate(129, 3, 7.0)])
    return c


EXACT = ("sc1", "bcc", "bcc_cap6", "fcc", "diamond", "sc64", "sc64_fine", "sc256", "dyadic", "n1", "n2", "n5", "n63",
         "n65", "n255", "ragged_1_between", "ragged_small", "cluster", "edgeless1", "edgeless_batch", "mixed_edgeless",
         "edgeless_run600", "hub_and_leaves", "fcc_cap18", "fcc_cap17", "n63_cap252") + tuple(f"sc64_cap{m}" for m in (1, 6, 12, 18, 0, -1, 256, 300))

# refusals: (natoms, frac, lattices, max_nb, knn_edges_per_atom) outside the library's limits
def refusal_cases():
    nat, x, L = _batch(SC64_FINE)
    fnat, fx, fL = _batch(FCC)
    return {"above_256_edges": (nat, x, L, 0, 512),      # uncapped: 304 edges on every node
            "above_capacity": (fnat, fx, fL, 20, 1)}     # fcc: 72 edges, capacity 4


@functools.lru_cache(maxsize=None)
def reference(name):
    nat, x, L, max_nb, _ = cases()[name]
    g = graph(nat, x, L, max_nb)
    for k in ("src", "dst", "fd", "deg"):
        g[k].setflags(write=False)
    return g


def segment_tiles(deg):
    """The node-aligned segment tiles knn_build cuts from the out-degrees: runs [first, last) of whole nodes with at
    most 256 edge rows and at most 256 nodes (edgeless nodes add no rows). Restated here so that the CPU test can say
    which tiles a case reaches."""
    tiles, cur0, rows = [], 0, 0
    for v, d in enumerate(deg):
        if rows + d > MAX_DEG or v - cur0 >= 256:
            tiles.append((cur0, v))
            cur0, rows = v, 0
        rows += int(d)
    tiles.append((cur0, len(deg)))
    return tiles


# ---------------------------------------------------------------- the message path on an explicit edge list

def fourier_args(fd):
    """arg [E, 3 NF] float32 of the given displacements (no % 1), as k_fourier_h rounds them: fl(fd fl(fl(2 pi) k))."""
    f = (np.float32(2.0 * np.pi) * np.arange(NF, dtype=np.float32)).astype(np.float32)
    fd = np.asarray(fd, np.float32)
    return (fd[:, :, None] * f[None, None, :]).astype(np.float32).reshape(len(fd), 3 * NF)


def msg_ref64(src, dst, fd, N, PQ, w):
    """agg [P, N, H] float64 on the edge list (src = i, dst = j, grouped by src):
    agg[c][i] = sum over i's edges of SiLU(SiLU(D f(fd) + P_c[i] + Q_c[j]) W2^T + b2) / max(deg_i, 1)."""
    PQ = np.asarray(PQ, np.float64)
    out = np.zeros((PQ.shape[0], N, H))
    if len(src) == 0:
        return out
    arg = fourier_args(fd).astype(np.float64)
    DF = np.concatenate([np.sin(arg), np.cos(arg)], 1) @ w["D"].astype(np.float64).T
    W2t, b2 = w["W2"].astype(np.float64).T, w["b2"].astype(np.float64)
    deg = np.bincount(src, minlength=N)
    for c in range(PQ.shape[0]):
        M = EC.silu64(EC.silu64(DF + PQ[c, src, :H] + PQ[c, dst, H:]) @ W2t + b2)
        np.add.at(out[c], src, M)
        out[c] /= np.maximum(deg, 1)[:, None]
    return out


def msg_base32(src, dst, fd, N, PQ, w):
    """The same chain in torch float32 on the CPU (the baseline of the gate, as edge_cases.base32)."""
    import torch
    import torch.nn.functional as F
    PQ = torch.tensor(np.asarray(PQ, np.float32))
    out = torch.zeros(PQ.shape[0], N, H)
    if len(src) == 0:
        return out.numpy()
    arg = torch.from_numpy(fourier_args(fd))
    DF = torch.cat([arg.sin(), arg.cos()], 1) @ torch.from_numpy(w["D"]).T
    W2, b2 = torch.from_numpy(w["W2"]), torch.from_numpy(w["b2"])
    ti, tj = torch.from_numpy(np.array(src)), torch.from_numpy(np.array(dst))
    deg = torch.bincount(ti, minlength=N).clamp(min=1).float()
    for c in range(PQ.shape[0]):
        M = F.silu(F.linear(F.silu(DF + PQ[c, ti, :H] + PQ[c, tj, H:]), W2, b2))
        out[c].index_add_(0, ti, M)
        out[c] /= deg[:, None]
    return out.numpy()
