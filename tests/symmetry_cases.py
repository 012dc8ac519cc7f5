"""Shared inputs of the crystal-system tests (chemeleon_amd.symmetry, csrc/symm.hip) and two numpy restatements of
the definition in include/chemeleon_hip.h at chm_symm_*:

  * `restate(case, dtype=np.float32)`: op for op what the device does: every product and sum is one rounded
    float32 numpy operation, in the header's order. The device records are pinned to it.
  * `restate(case, dtype=np.float64)`: the same definition in float64, which also reports the margin: the
    smallest relative distance of any distance test (every candidate (W, t_j), every atom i, every atom k of i's
    type, every level visited) from its tolerance.

Both take the lattice part (T, the reduced cell rounded to float32, the halvings and the accepted set {W}) from
the float64 restatement of the cell search, tests/cell_cases.py, whose own margin is part of the condition; both
start from the same float32 reduced coordinates x' = frac(x adj(T)) (float64, rounded once), so that what is left
to differ between the two is the arithmetic of the atom search, which the margin condition
(tests/test_symmetry_cases.py: MARGIN) keeps away from every decision.

The structures are built by applying a space group's generators (closed to the whole group) to stated positions,
so the expected point group holds by construction; EXPECTED lists what the issue's table states for them. No
restatement disagreed with a listed value.

Variants: every base case also under a random rotation, a random unimodular change of basis, a permutation of the
atoms and a shift of the origin (VARIANTS each); the record must come out the same. Variants that miss the margin
condition are dropped (at most 5%; dropped_variants() lists them).

Halving: find_halving() searched seeded displacements of the 8-atom rock-salt cell for a crystal whose accepted
set is no group at tol = symprec and that keeps the margin; HALVING is what it returned (case "one_halving").
"""

import functools
import math

import numpy as np

from tests import cell_cases as cc

CRYSTAL_SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")
TABLE = {(1, 0, 0, 0, 0): 0, (2, 1, 0, 0, 0): 1, (4, 3, 0, 0, 0): 2, (4, 1, 0, 2, 0): 3, (8, 5, 0, 2, 0): 3,
         (3, 0, 2, 0, 0): 4, (6, 3, 2, 0, 0): 4, (6, 1, 2, 0, 2): 5, (12, 7, 2, 0, 2): 5, (12, 3, 8, 0, 0): 6,
         (24, 9, 8, 6, 0): 6}
AMBIGUOUS, MISMATCH, NO_LATTICE, THIN = 1, 2, 4, 8
SYMPREC, ANGLE_TOLERANCE = 0.1, 10.0
MAX_HALVINGS, MAX_OPS = 4, 48
MARGIN = 1.0e-3
VARIANTS = 2
IDENTITY_INDEX = 16484
INT_FIELDS = ("system", "n_sym", "n_trans", "n_pg", "n_proper", "n2", "n3", "n4", "n6", "inversion", "halvings",
              "flags", "n_pivot", "lattice_system")


# ------------------------------------------------------------------------------------------ the restatements
def candidate_index(W) -> int:
    return int(sum((int(v) + 1) * 3 ** q for q, v in enumerate(np.asarray(W).reshape(9))))


def lattice_part(lattice, symprec=SYMPREC, angle_tolerance=ANGLE_TOLERANCE):
    """The cell record (tests/cell_cases.classify) and the accepted W [n,3,3] int64 with their candidate indices,
    ascending, at the record's final level; (record, None, None) where the record has no system."""
    rec = cc.classify(lattice, symprec, angle_tolerance)
    if rec["code"] < 0:
        return rec, None, None
    W, _, _ = cc.candidates()
    dl, da = cc.deviations(rec["lattice"].astype(np.float64))
    sp, at = float(np.float32(symprec)), float(np.float32(angle_tolerance))
    acc = (dl <= sp * 0.5 ** rec["halvings"]) & (da <= at * 0.5 ** rec["halvings"])
    Ws = W[acc]
    idx = np.array([candidate_index(w) for w in Ws])
    assert np.all(np.diff(idx) > 0) and len(Ws) == rec["counts"][0]
    return rec, Ws, idx


def reduced_coordinates(frac, T) -> np.ndarray:
    """x' = frac(x adj(T)) in float64, rounded once to float32, in [0, 1) (chm_cell_apply)."""
    T = np.asarray(T, dtype=np.int64)
    adj = np.round(np.linalg.inv(T.astype(np.float64)) * round(np.linalg.det(T.astype(np.float64)))).astype(np.int64)
    assert np.array_equal(adj @ T, np.eye(3, dtype=np.int64))
    x = np.asarray(frac, dtype=np.float32).astype(np.float64)
    a = adj.astype(np.float64)
    y = np.stack([(x[:, 0] * a[0, k] + x[:, 1] * a[1, k]) + x[:, 2] * a[2, k] for k in range(3)], axis=1)
    f = (y - np.floor(y)).astype(np.float32)
    f[f >= 1.0] = 0.0
    return f


def _xw(x, W, dt):
    """x W per atom, component k = (x0 W[0][k] + x1 W[1][k]) + x2 W[2][k], each operation rounded in dt."""
    W = W.astype(dt)
    return np.stack([(x[..., 0] * W[0, k] + x[..., 1] * W[1, k]) + x[..., 2] * W[2, k] for k in range(3)], axis=-1)


def _search(xr, types, Lr, Ws, pivots, tol, dt):
    """accepted [nW, n_pivot] (bool), t [nW, n_pivot, 3] and the smallest |dist - tol| / tol of all distance tests
    at tolerance tol (a dt scalar)."""
    x = xr.astype(dt)
    L = Lr.astype(dt)
    same = types[:, None] == types[None, :]
    n, npv = len(x), len(pivots)
    acc = np.zeros((len(Ws), npv), dtype=bool)
    ts = np.zeros((len(Ws), npv, 3), dtype=dt)
    margin = math.inf
    tol2 = dt(tol) * dt(tol)
    chunk = max(1, 2 ** 21 // (n * n))
    for w, W in enumerate(Ws):
        xw = _xw(x, W, dt)                                  # [n,3]
        t = x[pivots] - xw[pivots[0]][None, :]             # [npv,3]
        ts[w] = t
        for j0 in range(0, npv, chunk):
            tj = t[j0:j0 + chunk]
            y = xw[None, :, :] + tj[:, None, :]            # [c,n,3]
            d = y[:, :, None, :] - x[None, None, :, :]     # [c,n,n,3]
            d = d - np.rint(d)
            c = [(d[..., 0] * L[0, k] + d[..., 1] * L[1, k]) + d[..., 2] * L[2, k] for k in range(3)]
            r2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            ok = (r2 <= tol2) & same[None]
            acc[w, j0:j0 + chunk] = ok.any(axis=2).all(axis=1)
            if dt is np.float64:  # (the nearest distance below and above the tolerance)
                lo = np.where(ok, r2, -1.0).max()
                hi = np.where(same[None] & ~ok, r2, math.inf).min()
                for v in (lo, hi):
                    if 0 <= v < math.inf:
                        margin = min(margin, abs(math.sqrt(v) - float(tol)) / float(tol))
    return acc, ts, margin


def spacings(Lr, dt):
    L = Lr.astype(dt)
    a0, a1, a2 = L[0], L[1], L[2]

    def cross(u, v):
        return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=dt)

    def dot(u, v):
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    cs = [cross(a1, a2), cross(a2, a0), cross(a0, a1)]
    vol = abs(dot(a0, cs[0]))
    return [vol / np.sqrt(dot(c, c)) for c in cs]


def restate(case, dtype=np.float32, symprec=SYMPREC, angle_tolerance=ANGLE_TOLERANCE, require=-1):
    """The record of one case as a dict: INT_FIELDS, tol (float32), margin (float64 only: of the atom search),
    lattice_margin, ops (a list of (candidate index, t [3] in dtype) per accepted W, ascending) and, for the
    checks of the operations, Lr (float32), xr (float32), W_index (the accepted lattice set)."""
    dt = dtype
    out = dict.fromkeys(INT_FIELDS, 0)
    out.update(system=-1, lattice_system=-1, tol=np.float32(0), margin=math.inf, lattice_margin=math.inf, ops=[])
    sp = np.float32(symprec)

    def done():
        if require >= 0 and out["system"] != require:
            out["flags"] |= MISMATCH
        return out

    rec, Ws, idx = lattice_part(case["lattice"], symprec, angle_tolerance)
    out["lattice_margin"] = rec["margin"]
    if Ws is None:
        out["flags"] = NO_LATTICE
        return done()
    out["lattice_system"] = rec["code"]
    Lr = rec["lattice"]
    xr = reduced_coordinates(case["frac"], rec["transform"])
    out.update(Lr=Lr, xr=xr, W_index=idx)
    d = spacings(Lr, dt)
    if not dt(2) * dt(sp) < min(d):
        out["flags"] = THIN
        out["tol"] = sp
        return done()
    if dt is np.float64:
        out["margin"] = min(out["margin"], abs(float(min(d)) - 2 * float(sp)) / (2 * float(sp)))
    types = np.asarray(case["types"], dtype=np.int64)
    kinds, counts = np.unique(types, return_counts=True)       # (ascending types: the first minimum is the tie rule)
    ptype = kinds[np.argmin(counts)]
    pivots = np.flatnonzero(types == ptype)
    out["n_pivot"] = len(pivots)
    dets = np.round(np.linalg.det(Ws.astype(np.float64))).astype(np.int64)
    for h in range(MAX_HALVINGS + 1):
        tol = np.float32(sp * np.float32(0.5 ** h))
        acc, ts, margin = _search(xr, types, Lr, Ws, pivots, dt(tol), dt)
        out["margin"] = min(out["margin"], margin)
        has = acc.any(axis=1)
        proper = {}
        for w in np.flatnonzero(has):
            P = dets[w] * Ws[w]
            proper[candidate_index(P)] = int(np.trace(P))
        tr = list(proper.values())
        tup = (len(proper), tr.count(-1), tr.count(0), tr.count(1), tr.count(2))
        n_sym, n_pg = int(acc.sum()), int(has.sum())
        n_trans = int(acc[list(idx).index(IDENTITY_INDEX)].sum()) if IDENTITY_INDEX in idx else 0
        inv = int(any(idx[w] == 3 ** 9 - 1 - IDENTITY_INDEX for w in np.flatnonzero(has)))
        out.update(n_sym=n_sym, n_trans=n_trans, n_pg=n_pg, n_proper=tup[0], n2=tup[1], n3=tup[2], n4=tup[3], n6=tup[4],
                   inversion=inv, halvings=h, tol=tol,
                   ops=[(int(idx[w]), ts[w, int(np.argmax(acc[w]))].copy()) for w in np.flatnonzero(has)])
        if tup in TABLE and n_sym == n_pg * n_trans and n_pg == tup[0] * (1 + inv):
            out["system"] = TABLE[tup]
            break
    else:
        out["flags"] |= AMBIGUOUS
    return done()


# ------------------------------------------------------------------------------------------ building structures
def _closure(generators):
    """The group generated by (R [3,3] int, t [3]) acting on fractional columns x -> R x + t, translations mod 1."""
    def key(R, t):
        return tuple(R.reshape(9)) + tuple(np.round(np.mod(np.round(t * 24) / 24, 1.0) * 24).astype(int) % 24)

    ops = {}
    todo = [(np.eye(3, dtype=np.int64), np.zeros(3))]
    gens = [(np.array(R, dtype=np.int64), np.array(t, dtype=np.float64)) for R, t in generators]
    while todo:
        R, t = todo.pop()
        k = key(R, t)
        if k in ops:
            continue
        ops[k] = (R, np.mod(t, 1.0))
        assert len(ops) <= 192 * 4
        for G, s in gens:
            todo.append((G @ R, G @ t + s))
    return list(ops.values())


def _orbit(ops, pos):
    pts = []
    for R, t in ops:
        p = np.mod(R @ np.asarray(pos, dtype=np.float64) + t, 1.0)
        p[np.abs(p - 1.0) < 1e-9] = 0.0
        if not any(np.abs((p - q) - np.rint(p - q)).max() < 1e-6 for q in pts):
            pts.append(p)
    return pts


def build(lattice, generators, sites):
    """(lattice [3,3] float64, types [N], frac [N,3] float64): the orbits of `sites` = [(type, position), ...]
    under the group closed from `generators`."""
    ops = _closure(generators)
    types, frac = [], []
    for z, pos in sites:
        for p in _orbit(ops, pos):
            types.append(z)
            frac.append(p)
    return np.asarray(lattice, dtype=np.float64), np.array(types, dtype=np.int64), np.array(frac)


E = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
INV = ([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], [0, 0, 0])
FOUR_Z = ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [0, 0, 0])          # (-y, x, z)
THREE_111 = ([[0, 0, 1], [1, 0, 0], [0, 1, 0]], [0, 0, 0])       # (z, x, y)
TWO_Z = ([[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [0, 0, 0])
TWO_Y = ([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], [0, 0, 0])
MIRROR_XY = ([[0, 1, 0], [1, 0, 0], [0, 0, 1]], [0, 0, 0])       # (y, x, z)
FCC_CENTRING = [(E, [0, .5, .5]), (E, [.5, 0, .5])]
THREE_HEX = [[0, -1, 0], [1, -1, 0], [0, 0, 1]]                   # (-y, x - y, z)
FCC_PRIMITIVE = lambda a: 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0.0]])  # noqa: E731

# name -> (system, n_pg, inversion, n_trans): the table of the issue
EXPECTED = {
    "simple_cubic": ("cubic", 48, 1, 1), "cscl": ("cubic", 48, 1, 1), "rocksalt8": ("cubic", 48, 1, 4),
    "rocksalt_primitive": ("cubic", 48, 1, 1), "diamond_primitive": ("cubic", 48, 1, 1),
    "zincblende_primitive": ("cubic", 24, 0, 1), "pyrite": ("cubic", 24, 1, 1), "rutile": ("tetragonal", 16, 1, 1),
    "hcp": ("hexagonal", 24, 1, 1), "wurtzite": ("hexagonal", 12, 0, 1), "quartz": ("trigonal", 6, 0, 1),
    "r3m_bar": ("trigonal", 12, 1, 1), "ortho_mmm": ("orthorhombic", 8, 1, 1), "mono_2m": ("monoclinic", 4, 1, 1),
    "p1_bar": ("triclinic", 2, 1, 1), "p1": ("triclinic", 1, 0, 1), "cubic_general5": ("triclinic", 1, 0, 1),
    "cscl_2x1x1": ("tetragonal", 16, 1, 2),
}
EXPECTED_LATTICE = {"quartz": "hexagonal", "cubic_general5": "cubic", "r3m_bar": "rhombohedral"}


def _supercell_sc(a, reps, skip_first=False):
    n0, n1, n2 = reps
    frac = np.array([[i / n0, j / n1, k / n2] for i in range(n0) for j in range(n1) for k in range(n2)])
    if skip_first:
        frac = frac[1:]
    return np.diag([a * n0, a * n1, a * n2]).astype(np.float64), np.full(len(frac), 29, dtype=np.int64), frac


def _base_structures():
    out = {}
    cub = lambda a: cc.cell(a, a, a, 90, 90, 90)  # noqa: E731
    out["simple_cubic"] = build(cub(3.0), [], [(84, [0, 0, 0])])
    out["cscl"] = build(cub(4.1), [FOUR_Z, THREE_111, INV], [(55, [0, 0, 0]), (17, [.5, .5, .5])])
    out["rocksalt8"] = build(cub(5.6), [FOUR_Z, THREE_111, INV] + FCC_CENTRING, [(11, [0, 0, 0]), (17, [.5, .5, .5])])
    out["rocksalt_primitive"] = build(FCC_PRIMITIVE(5.6), [INV], [(11, [0, 0, 0]), (17, [.5, .5, .5])])
    out["diamond_primitive"] = build(FCC_PRIMITIVE(3.57), [([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], [.25, .25, .25])],
                                     [(6, [0, 0, 0])])
    out["zincblende_primitive"] = build(FCC_PRIMITIVE(5.41), [], [(30, [0, 0, 0]), (16, [.25, .25, .25])])
    out["pyrite"] = build(cub(5.42), [([[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [.5, 0, .5]),
                                      ([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], [0, .5, .5]), THREE_111, INV],
                          [(26, [0, 0, 0]), (16, [.385, .385, .385])])
    out["rutile"] = build(cc.cell(4.59, 4.59, 2.96, 90, 90, 90),
                          [TWO_Z, ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [.5, .5, .5]),
                           ([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], [.5, .5, .5]), INV],
                          [(22, [0, 0, 0]), (8, [.305, .305, 0])])
    hexc = lambda a, c: cc.cell(a, a, c, 90, 90, 120)  # noqa: E731
    out["hcp"] = build(hexc(3.2, 5.2), [(THREE_HEX, [0, 0, 0]), (TWO_Z[0], [0, 0, .5]),
                                        ([[0, 1, 0], [1, 0, 0], [0, 0, -1]], [0, 0, 0]), INV],
                       [(12, [1 / 3, 2 / 3, .25])])
    out["wurtzite"] = build(hexc(3.82, 6.26), [(THREE_HEX, [0, 0, 0]), (TWO_Z[0], [0, 0, .5]),
                                               ([[0, -1, 0], [-1, 0, 0], [0, 0, 1]], [0, 0, 0])],
                            [(30, [1 / 3, 2 / 3, 0]), (16, [1 / 3, 2 / 3, .375])])
    out["quartz"] = build(hexc(4.916, 5.405), [(THREE_HEX, [0, 0, 1 / 3]), ([[0, 1, 0], [1, 0, 0], [0, 0, -1]], [0, 0, 0])],
                          [(14, [.4697, 0, 1 / 3]), (8, [.4135, .2669, .1191])])
    out["r3m_bar"] = build(cc.cell(5, 5, 5, 72, 72, 72), [THREE_111, ([[0, -1, 0], [-1, 0, 0], [0, 0, -1]], [0, 0, 0]), INV],
                           [(83, [0, 0, 0]), (52, [.24, .24, .24])])
    out["ortho_mmm"] = build(cc.cell(4, 5.2, 6.7, 90, 90, 90), [TWO_Z, TWO_Y, INV],
                             [(20, [0, 0, 0]), (8, [.13, .21, .37])])
    out["mono_2m"] = build(cc.cell(4.0, 5.3, 6.7, 90, 104, 90), [TWO_Y, INV], [(20, [0, 0, 0]), (8, [.13, .21, .37])])
    tri = cc.cell(4.0, 5.3, 6.7, 78, 97, 109)
    out["p1_bar"] = build(tri, [INV], [(20, [0, 0, 0]), (8, [.13, .21, .37])])
    out["p1"] = build(tri, [], [(20, [.05, .1, .2]), (8, [.13, .51, .37]), (6, [.62, .33, .81])])
    out["cubic_general5"] = build(cub(5.3), [], [(29, p) for p in ([.05, .11, .23], [.31, .62, .17], [.55, .29, .71],
                                                                 [.83, .47, .39], [.19, .88, .64])])
    out["cscl_2x1x1"] = (np.diag([8.2, 4.1, 4.1]), np.array([55, 55, 17, 17]),
                         np.array([[0, 0, 0], [.5, 0, 0], [.25, .5, .5], [.75, .5, .5]]))
    return out


def _displaced(struct, amplitude, seed):
    L, types, frac = struct
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(frac.shape)
    v *= amplitude / np.linalg.norm(v, axis=1, keepdims=True)
    return L, types, np.mod(frac + v @ np.linalg.inv(L), 1.0)


def find_halving(trials=200, seed=11):
    """A seeded search for displacements of the 8-atom rock-salt cell whose accepted set is no group at
    tol = symprec (a halving is needed) and that keep twice the margin; (seed, amplitude) or None."""
    base = _base_structures()["rocksalt8"]
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        s, amp = int(rng.integers(1 << 30)), float(rng.uniform(0.02, 0.07))
        L, types, frac = _displaced(base, amp, s)
        case = dict(lattice=L.astype(np.float32), types=types, frac=frac.astype(np.float32))
        r = restate(case, np.float64)
        if r["halvings"] >= 1 and r["flags"] == 0 and min(r["margin"], r["lattice_margin"]) >= 2 * MARGIN:
            return s, amp
    return None


HALVING = (780730290, 0.06264599972272639)  # (seed, amplitude) that find_halving() returns within its 200 trials


def _variant(struct, rng):
    L, types, frac = struct
    U, Q = cc.unimodular(rng), cc.rotation(rng)
    Ui = np.round(np.linalg.inv(U.astype(np.float64))).astype(np.int64)
    assert np.array_equal(Ui @ U, np.eye(3, dtype=np.int64))
    perm = rng.permutation(len(types))
    x = np.mod(frac @ Ui.astype(np.float64) + rng.random(3), 1.0)
    return U.astype(np.float64) @ L @ Q, types[perm], x[perm]


def _case(name, struct, family=None):
    L, types, frac = struct
    return dict(name=name, family=family or name, lattice=np.asarray(L, dtype=np.float32).reshape(3, 3),
                types=np.asarray(types, dtype=np.int64), frac=np.mod(np.asarray(frac, dtype=np.float32), np.float32(1)))


@functools.lru_cache(maxsize=None)
def _all_cases():
    """(kept cases, names of the dropped variants)."""
    kept, dropped = [], []
    rng = np.random.default_rng(20261020)
    base = _base_structures()
    for name, struct in base.items():
        kept.append(_case(name, struct))
        for v in range(VARIANTS):
            c = _case(f"{name}_v{v}", _variant(struct, rng), family=name)
            r = restate(c, np.float64)
            if min(r["margin"], r["lattice_margin"]) < MARGIN:
                dropped.append(c["name"])
            else:
                kept.append(c)
    kept.append(_case("rocksalt8_d002", _displaced(base["rocksalt8"], 0.02, 5)))
    kept.append(_case("rocksalt8_d04", _displaced(base["rocksalt8"], 0.4, 6)))
    if HALVING is not None:
        kept.append(_case("one_halving", _displaced(base["rocksalt8"], HALVING[1], HALVING[0])))
    # sizes at the wave and block edges (N = 1 and 2 are simple_cubic and cscl)
    kept.append(_case("sc_63", _supercell_sc(3.0, (4, 4, 4), skip_first=True)))
    kept.append(_case("sc_64", _supercell_sc(3.0, (4, 4, 4))))
    L, types, frac = _supercell_sc(3.0, (4, 4, 4))
    kept.append(_case("sc_65", (L, np.append(types, 8), np.vstack([frac, [[.125, .125, .125]]]))))
    kept.append(_case("sc_256", _supercell_sc(3.0, (4, 8, 8))))
    kept.append(_case("thin", (cc.cell(4, 5.2, 0.19, 90, 90, 90), [29], [[0, 0, 0]])))
    kept.append(_case("no_lattice", ([[4.0, 0, 0], [0, float("nan"), 0], [0, 0, 5.0]], [29, 8], [[0, 0, 0], [.5, .5, .5]])))
    return kept, dropped


def cases():
    return _all_cases()[0]


def dropped_variants():
    return _all_cases()[1]


SIZE_EXPECTED = {"sc_63": ("cubic", 48, 1, 1, 63), "sc_64": ("cubic", 48, 1, 64, 64), "sc_65": ("cubic", 48, 1, 1, 1),
                 "sc_256": ("tetragonal", 16, 1, 256, 256)}  # system, n_pg, inversion, n_trans, n_pivot


@functools.lru_cache(maxsize=None)
def _reference(dtype_name):
    dt = np.float32 if dtype_name == "float32" else np.float64
    return [restate(c, dt) for c in cases()]


def reference(dtype_name="float32", require=-1):
    """The records of cases() in float32 or float64, computed once (shared; do not modify). With a required
    code, the same records with MISMATCH set where the system is another (what restate(require=) gives)."""
    if require >= 0:
        return [dict(r, flags=r["flags"] | (MISMATCH if r["system"] != require else 0)) for r in _reference(dtype_name)]
    return _reference(dtype_name)


def state(indices):
    """(natoms, types int64 [N], frac float32 [N,3], lattices float32 [B,3,3]) of the cases `indices`, as numpy."""
    cs = cases()
    nat = [len(cs[k]["types"]) for k in indices]
    return (nat, np.concatenate([cs[k]["types"] for k in indices]), np.concatenate([cs[k]["frac"] for k in indices]),
            np.stack([cs[k]["lattice"] for k in indices]))


def batch(B):
    """The indices into cases() of a batch of B crystals: the flagged and the edge cases first, then the rest in
    order, cycling; the 256-atom case only once."""
    cs = cases()
    first = [k for name in ("quartz", "no_lattice", "thin", "sc_65", "sc_64", "sc_63", "rocksalt8_d04")
             for k, c in enumerate(cs) if c["name"] == name]
    rest = [k for k, c in enumerate(cs) if k not in first and c["name"] != "sc_256"]
    order = first + rest
    return [order[k % len(order)] for k in range(B)]
