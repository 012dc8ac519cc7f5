"""Shared inputs of the primitive-cell tests (chemeleon_amd.primitive, csrc/prim.hip) and two numpy restatements
of the definition in include/chemeleon_hip.h at chm_prim_*:

  * `restate(case, dtype=np.float32)`: op for op what the device does: every product and sum of the search is
    one rounded float32 numpy operation, in the header's order. The device output is pinned to it, bit for bit.
  * `restate(case, dtype=np.float64)`: the same definition with the search in float64, which also reports the
    margin: the smallest relative distance of any distance test (every candidate t_j, every atom i, every atom k
    of i's type, every t_j against q_j / m, every level visited) from its tolerance, and of 2 symprec from the
    smallest plane spacing.

Both take the lattice part from the float64 restatement of the cell search (tests/symmetry_cases.lattice_part)
and start from the same float32 reduced coordinates, as the symmetry restatements do; the Hermite normal form is
computed in Python integers by row elimination over all generators at once, which is another order of reduction
than the device's one-generator-at-a-time update: H is unique, so they must agree. Lp and x_p are float64
expressions of float32 inputs and integers, rounded once, in both restatements.

The cases are the smallest shapes at which the reduction can go wrong (EXPECTED: name -> (n, n_prim, m)), each
also under VARIANTS seeded variants (rotation, unimodular change of basis, permutation, origin shift:
symmetry_cases._variant). Variants that miss the margin condition are dropped (dropped_variants() lists them);
the named cases are never dropped: tests/test_prim_cases.py asserts their margins.
"""

import functools
import math

import numpy as np

from tests import cell_cases as cc
from tests import symmetry_cases as S

AMBIGUOUS, NO_LATTICE, THIN = 1, 4, 8
SYMPREC, ANGLE_TOLERANCE = S.SYMPREC, S.ANGLE_TOLERANCE
MAX_HALVINGS = S.MAX_HALVINGS
MARGIN = S.MARGIN
VARIANTS = 2
INT_FIELDS = ("n_prim", "n_trans", "n_pivot", "halvings", "flags", "h00", "h01", "h02", "h11", "h12", "h22")
# (the record's int32 words 0..10; word 11 is tol, word 12 lattice_system, 13..15 are 0)


# ------------------------------------------------------------------------------------------ integers
def hnf(rows):
    """The row Hermite normal form [3][3] (Python ints) of the lattice spanned by integer rows of full rank: upper
    triangular, positive diagonal, 0 <= H[i][k] < H[k][k] for i < k."""
    rows = [[int(v) for v in r] for r in rows if any(int(v) != 0 for v in r)]
    H = []
    for col in range(3):
        while True:
            nz = [r for r in rows if r[col] != 0]
            if len(nz) <= 1:
                break
            piv = min(nz, key=lambda r: abs(r[col]))
            for r in nz:
                if r is not piv:
                    f = r[col] // piv[col]
                    for k in range(3):
                        r[k] -= f * piv[k]
        assert nz, "the generators do not have full rank"
        piv = nz[0]
        rows = [r for r in rows if r is not piv and any(r)]
        H.append([-v for v in piv] if piv[col] < 0 else piv)
    for k in (1, 2):
        for i in range(k):
            f = H[i][k] // H[k][k]
            for c in range(3):
                H[i][c] -= f * H[k][c]
    return H


def adjugate(M):
    """adj(M) [3][3] in Python ints: M adj(M) = det(M) I."""
    t = [int(v) for row in M for v in row]
    return [[t[4] * t[8] - t[5] * t[7], t[2] * t[7] - t[1] * t[8], t[1] * t[5] - t[2] * t[4]],
            [t[5] * t[6] - t[3] * t[8], t[0] * t[8] - t[2] * t[6], t[2] * t[3] - t[0] * t[5]],
            [t[3] * t[7] - t[4] * t[6], t[1] * t[6] - t[0] * t[7], t[0] * t[4] - t[1] * t[3]]]


# ------------------------------------------------------------------------------------------ the restatements
def _close(d, L, tol2):
    """(r2 <= tol2, r2) of the distance test on differences d [...,3] (the device's lands_on, after d = y - b)."""
    d = d - np.rint(d)
    c = [(d[..., 0] * L[0, k] + d[..., 1] * L[1, k]) + d[..., 2] * L[2, k] for k in range(3)]
    r2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    return r2 <= tol2, r2


def _rel(r2, tol):
    return abs(math.sqrt(float(r2)) - float(tol)) / float(tol)


def restate(case, dtype=np.float32, symprec=SYMPREC, angle_tolerance=ANGLE_TOLERANCE):
    """One case as a dict: INT_FIELDS, lattice_system, tol (float32), margin and lattice_margin (float64 only
    meaningful), H [3][3] ints, Lr / xr (the reduced basis, float32), keep (the kept node indices), and the output
    Lp [3,3] float32, xp [n_prim,3] float32, types_p [n_prim] int64."""
    dt = dtype
    out = dict.fromkeys(INT_FIELDS, 0)
    n = len(case["types"])
    types = np.asarray(case["types"], dtype=np.int64)
    out.update(n_prim=n, h00=1, h11=1, h22=1, lattice_system=-1, tol=np.float32(0), margin=math.inf,
               lattice_margin=math.inf, H=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], keep=np.arange(n))
    sp = np.float32(symprec)
    rec, Ws, idx = S.lattice_part(case["lattice"], symprec, angle_tolerance)
    out["lattice_margin"] = rec["margin"]
    Lr = rec["lattice"]
    xr = S.reduced_coordinates(case["frac"], rec["transform"])
    out.update(Lr=Lr, xr=xr, Lp=Lr.copy(), xp=xr.copy(), types_p=types.copy())
    if Ws is None:
        out["flags"] = NO_LATTICE
        return out
    out["lattice_system"] = rec["code"]
    d = S.spacings(Lr, dt)
    if not dt(2) * dt(sp) < min(d):
        out["flags"] = THIN
        out["tol"] = sp
        return out
    if dt is np.float64:
        out["margin"] = abs(float(min(d)) - 2 * float(sp)) / (2 * float(sp))
    kinds, counts = np.unique(types, return_counts=True)       # (ascending types: the first minimum is the tie rule)
    ptype = kinds[np.argmin(counts)]
    pivots = np.flatnonzero(types == ptype)
    out["n_pivot"] = len(pivots)
    x, L = xr.astype(dt), Lr.astype(dt)
    same = types[:, None] == types[None, :]
    below = np.tri(n, k=-1, dtype=bool)                        # [i, k]: k < i
    eye = np.eye(3, dtype=np.int64)[None]
    consistent = False
    for h in range(MAX_HALVINGS + 1):
        tol = np.float32(sp * np.float32(0.5 ** h))
        tol2 = dt(tol) * dt(tol)
        acc, ts, margin = S._search(xr, types, Lr, eye, pivots, dt(tol), dt)
        out["margin"] = min(out["margin"], margin)
        acc, ts = acc[0], ts[0]
        m = int(acc.sum())
        out.update(n_trans=m, halvings=h, tol=tol)
        if m == 0:
            continue
        t = ts[acc]                                            # [m,3], in pivot order
        q = np.rint(dt(m) * t).astype(np.int64) % m
        ok_c, r2 = _close(t - q.astype(dt) / dt(m), L, tol2)   # (c)
        if dt is np.float64:
            out["margin"] = min(out["margin"], min(_rel(v, tol) for v in r2))
        lower = np.zeros(n, dtype=bool)                        # (d): some partner(i, j) < i
        for tj in t:
            ok, _ = _close((x + tj[None, :])[:, None, :] - x[None, :, :], L, tol2)
            lower |= (ok & same & below).any(axis=1)
        keep = np.flatnonzero(~lower)
        H = hnf([list(v) for v in q] + [[m, 0, 0], [0, m, 0], [0, 0, m]])
        consistent = (bool(np.all(counts % m == 0)) and H[0][0] * H[1][1] * H[2][2] == m * m and bool(ok_c.all())
                      and len(keep) * m == n)
        if consistent:
            break
    if not consistent:
        out["flags"] = AMBIGUOUS
        return out
    if m == 1:
        return out
    out.update(n_prim=n // m, H=H, keep=keep, h00=H[0][0], h01=H[0][1], h02=H[0][2], h11=H[1][1], h12=H[1][2],
               h22=H[2][2])
    L64, fm = Lr.astype(np.float64), float(m)
    Hf = np.array(H, dtype=np.float64)
    out["Lp"] = np.array([[((Hf[i, 0] * L64[0, k] + Hf[i, 1] * L64[1, k]) + Hf[i, 2] * L64[2, k]) / fm
                           for k in range(3)] for i in range(3)], dtype=np.float64).astype(np.float32)
    A = np.array(adjugate(H), dtype=np.float64)
    x64 = xr[keep].astype(np.float64)
    y = np.stack([((x64[:, 0] * A[0, k] + x64[:, 1] * A[1, k]) + x64[:, 2] * A[2, k]) / fm for k in range(3)], axis=1)
    f = (y - np.floor(y)).astype(np.float32)
    f[f >= 1.0] = 0.0
    out.update(xp=f, types_p=types[keep].copy())
    return out


# ------------------------------------------------------------------------------------------ the cases
def _cscl(reps, a=4.1):
    n0, n1, n2 = reps
    cells = [(i, j, k) for i in range(n0) for j in range(n1) for k in range(n2)]
    frac = [[(i + o) / n0, (j + o) / n1, (k + o) / n2] for o in (0.0, 0.5) for i, j, k in cells]
    return (np.diag([a * n0, a * n1, a * n2]).astype(np.float64), np.array([55] * len(cells) + [17] * len(cells)),
            np.array(frac))


def _diamond8(a=3.57):
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    return cc.cell(a, a, a, 90, 90, 90), np.full(8, 6), np.vstack([fcc, fcc + 0.25])


def _one_displaced(struct, index, amplitude, seed):
    L, types, frac = struct
    v = np.random.default_rng(seed).standard_normal(3)
    v *= amplitude / np.linalg.norm(v)
    frac = np.array(frac, dtype=np.float64)
    frac[index] = np.mod(frac[index] + v @ np.linalg.inv(L), 1.0)
    return L, types, frac


def find_halving(trials=200, seed=11):
    """A seeded search for displacements of the 8-atom rock-salt cell whose accepted translations are no
    consistent set at tol = symprec (a halving is needed) and that keep twice the margin; (seed, amplitude) or
    None. The halving case of the symmetry tests (symmetry_cases.HALVING, case "one_halving" here) loses every
    translation at the first level already, so it does not reach the halving of this search; this one does."""
    base = S._base_structures()["rocksalt8"]
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        s, amp = int(rng.integers(1 << 30)), float(rng.uniform(0.03, 0.06))
        r = restate(S._case("trial", S._displaced(base, amp, s)), np.float64)
        if r["halvings"] >= 1 and r["flags"] == 0 and min(r["margin"], r["lattice_margin"]) >= 2 * MARGIN:
            return s, amp
    return None


HALVING = (588145293, 0.03389321848197894)  # (seed, amplitude) that find_halving() returns within its 200 trials

# name -> (n, n_prim, m): the table of the issue
EXPECTED = {
    "one_atom": (1, 1, 1), "cscl": (2, 2, 1), "cscl_2x1x1": (4, 2, 2), "cscl_3x1x1": (6, 2, 3),
    "cscl_2x2x1": (8, 2, 4), "cscl_2x3x1": (12, 2, 6), "bcc_conventional": (2, 1, 2), "rocksalt8": (8, 2, 4),
    "diamond8": (8, 2, 4), "sc_2x2x2": (8, 1, 8), "sc_64": (64, 1, 64), "sc_256": (256, 1, 256),
    "rutile": (6, 6, 1), "quartz": (9, 9, 1), "pyrite": (12, 12, 1),
    "rocksalt8_d002": (8, 2, 4),   # all atoms displaced by 0.02 A: the centring is kept
    "rocksalt8_one04": (8, 8, 1),  # one atom displaced by 0.4 A: the centring is lost
}


def _base_structures():
    sym = S._base_structures()
    out = {"one_atom": sym["simple_cubic"], "cscl": sym["cscl"], "cscl_2x1x1": sym["cscl_2x1x1"]}
    for reps in ((3, 1, 1), (2, 2, 1), (2, 3, 1)):
        out["cscl_%dx%dx%d" % reps] = _cscl(reps)
    out["bcc_conventional"] = (cc.cell(2.87, 2.87, 2.87, 90, 90, 90), np.array([26, 26]),
                               np.array([[0, 0, 0], [.5, .5, .5]]))
    out["rocksalt8"] = sym["rocksalt8"]
    out["diamond8"] = _diamond8()
    out["sc_2x2x2"] = S._supercell_sc(3.0, (2, 2, 2))
    out["sc_64"] = S._supercell_sc(3.0, (4, 4, 4))
    out["sc_256"] = S._supercell_sc(3.0, (4, 8, 8))
    for name in ("rutile", "quartz", "pyrite"):
        out[name] = sym[name]
    return out


@functools.lru_cache(maxsize=None)
def _all_cases():
    """(kept cases, names of the dropped variants)."""
    kept, dropped = [], []
    rng = np.random.default_rng(20261021)
    base = _base_structures()
    for name, struct in base.items():
        kept.append(S._case(name, struct))
        for v in range(VARIANTS):
            c = S._case(f"{name}_v{v}", S._variant(struct, rng), family=name)
            r = restate(c, np.float64)
            if min(r["margin"], r["lattice_margin"]) < MARGIN:
                dropped.append(c["name"])
            else:
                kept.append(c)
    kept.append(S._case("rocksalt8_d002", S._displaced(base["rocksalt8"], 0.02, 5)))
    kept.append(S._case("rocksalt8_one04", _one_displaced(base["rocksalt8"], 0, 0.4, 6)))
    kept.append(S._case("one_halving", S._displaced(base["rocksalt8"], S.HALVING[1], S.HALVING[0])))
    kept.append(S._case("prim_halving", S._displaced(base["rocksalt8"], HALVING[1], HALVING[0])))
    kept.append(S._case("thin", (cc.cell(4, 5.2, 0.19, 90, 90, 90), [29], [[0, 0, 0]])))
    kept.append(S._case("no_lattice", ([[4.0, 0, 0], [0, float("nan"), 0], [0, 0, 5.0]], [29, 8], [[0, 0, 0], [.5, .5, .5]])))
    return kept, dropped


def cases():
    return _all_cases()[0]


def dropped_variants():
    return _all_cases()[1]


@functools.lru_cache(maxsize=None)
def _reference(dtype_name):
    dt = np.float32 if dtype_name == "float32" else np.float64
    return [restate(c, dt) for c in cases()]


def reference(dtype_name="float32"):
    """The restatements of cases() in float32 or float64, computed once (shared; do not modify)."""
    return _reference(dtype_name)


def state(indices):
    """(natoms, types int64 [N], frac float32 [N,3], lattices float32 [B,3,3]) of the cases `indices`, as numpy."""
    cs = cases()
    nat = [len(cs[k]["types"]) for k in indices]
    return (nat, np.concatenate([cs[k]["types"] for k in indices]), np.concatenate([cs[k]["frac"] for k in indices]),
            np.stack([cs[k]["lattice"] for k in indices]))


def index_of(name):
    return next(k for k, c in enumerate(cases()) if c["name"] == name)
