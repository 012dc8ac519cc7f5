"""Shared inputs of the tests of pairing by assignment (Match / MatchDedup / MatchSet with pairing="assignment",
csrc/match.hip) and the numpy restatement of its definition in include/chemeleon_hip.h at chm_match_*:

  * `restate_assign(sample, ref, np.float64)`: frames, mappings and anchors as tests/match_cases.restate (the same
    helpers), then the prefilter (every reference atom has a same-type sample atom within c; no collision rule), the
    nearest partners where they are all different, else the type-preserving assignment of minimal sum |D|^2 by its
    own shortest-augmenting-path solver (`solve`; ties to the smallest column, as the device breaks them; not scipy),
    at most `max_assign` collided candidates, the lowest first.
  * `restate_assign(sample, ref, np.float32)`: the same with one rounded float32 operation per product and sum.

Besides the fields of match_cases.restate it reports n_assigned, the winner's `collided`, `perm` and `assign_gap`
(float64: second-best minus best assignment cost of the winner, in units of c^2; inf for a winner without collision),
`longest_path` (columns on the longest augmenting path of any solve: 1 + the rows it placed again), `rms_margin`, and
the margins of match_cases.restate of the same pair (`nearest`: its whole record under the nearest rule).

Cases (cases()): the three-atom cell of two close Cl sites whose nearest partners collide; the same collision put
into rutile and rock-salt (two species blocks, the second at an offset); a cell with species blocks of one atom;
simple-cubic supercells of 63, 64, 65 and 256 atoms with one collided pair and every other atom displaced by 0.05 A;
a chain whose augmenting path places two placed rows again; a symmetric cell with 16 collided candidates; a
supercell of it with more than MAX_ASSIGN of them; a sample that fails the prefilter; a NaN coordinate.
"""

import functools
import math

import numpy as np

from tests import cell_cases as cc
from tests import match_cases as mc
from tests import symmetry_cases as sc

MANY_ASSIGNMENTS = 128
MAX_ASSIGN = 64
INT_FIELDS = mc.INT_FIELDS + ("n_assigned",)


# ------------------------------------------------------------------------------------------ the solver
def solve(cost, same):
    """The bijection rows -> columns within `same` [k,i] of minimal total `cost` [k,i] (any float dtype; entries
    outside `same` are not read) by shortest augmenting paths from the dual start u = row minima, v = 0 with the
    non-colliding row minima placed (a column keeps its smallest row). Returns (col [k], longest path) or None when
    a row finds no column (NaN / Inf). Every comparison is the device's: strict, ties to the smallest column."""
    n = len(cost)
    dt = cost.dtype.type
    inf = dt(np.inf)
    seen = np.where(same & ~np.isnan(cost), cost, inf)
    bi = seen.argmin(axis=1)
    u = seen[np.arange(n), bi].copy()
    if not np.all(u < inf):
        return None
    v = np.zeros(n, dtype=cost.dtype)
    row_of_col, col = np.full(n, -1), np.full(n, -1)
    for k in range(n):
        if row_of_col[bi[k]] < 0:
            row_of_col[bi[k]], col[k] = k, bi[k]
    longest = 0
    for i in range(n):
        if col[i] >= 0:
            continue
        minv, way, used = np.full(n, inf, dtype=cost.dtype), np.full(n, -1), np.zeros(n, dtype=bool)
        i0, j0, reached = i, -1, False
        for _ in range(n):
            free = same[i] & ~used
            with np.errstate(invalid="ignore"):
                cur = (cost[i0] - u[i0]) - v
                upd = free & (cur < minv)
            minv[upd], way[upd] = cur[upd], j0
            open_ = np.where(free, minv, inf)
            j1 = int(open_.argmin())
            if not open_[j1] < inf:
                break
            delta = open_[j1]
            u[i] += delta
            u[row_of_col[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            used[j1] = True
            j0 = j1
            if row_of_col[j1] < 0:
                reached = True
                break
            i0 = row_of_col[j1]
        if not reached:
            return None
        j, length = j0, 0
        while j >= 0:
            jp = way[j]
            row = i if jp < 0 else row_of_col[jp]
            row_of_col[j], col[row] = row, j
            j, length = jp, length + 1
        longest = max(longest, length)
    return col, longest


def second_best(cost, same, col):
    """The smallest total cost of a bijection that differs from `col` (float64): the best over "edge (k, col[k])
    forbidden", every k of a species block of more than one atom. inf if there is no other bijection."""
    best = math.inf
    for k in range(len(col)):
        if same[k].sum() < 2:
            continue
        c2 = cost.copy()
        c2[k, col[k]] = 1e30
        other = solve(c2, same)
        if other is not None and other[0][k] != col[k]:
            best = min(best, float(c2[np.arange(len(col)), other[0]].sum()))
    return best


# ------------------------------------------------------------------------------------------ the restatement
def restate_assign(sample, ref, dtype=np.float64, ref_index=0, ltol=mc.LTOL, stol=mc.STOL, angle_tol=mc.ANGLE_TOL,
                   max_assign=MAX_ASSIGN):
    dt = dtype
    near = mc.restate(sample, ref, np.float64, ref_index, ltol, stol, angle_tol)
    out = dict(rms=0.0, max_dist=0.0, scale=near["scale"], l=near["l"], mapping=-1, anchor=-1,
               n_mappings=near["n_mappings"], n_candidates=near["n_candidates"], n_survivors=0, n_assigned=0, matched=0,
               flags=near["flags"], ref=near["ref"], counting=[], collided=False, perm=None, assign_gap=math.inf,
               longest_path=0, rms_margin=math.inf, pair_margin=math.inf, gap_margin=math.inf, nearest=near,
               lattice_margin=near["lattice_margin"], thin_margin=near["thin_margin"])
    if near["flags"] & ~mc.MANY_MAPPINGS:
        return out
    (Ts, Ls), (Tr, Lr) = mc.reduced(sample["lattice"]), mc.reduced(ref["lattice"])
    ts, tr = np.asarray(sample["types"], dtype=np.int64), np.asarray(ref["types"], dtype=np.int64)
    n = len(tr)
    scale, ell = dt(np.float32(out["scale"])), dt(np.float32(out["l"]))
    c = dt(np.float32(stol)) * ell
    c2 = c * c
    idx, W, _ = mc._candidates()
    sL = scale * Ls.astype(dt)
    lr, ar = mc._metric(Lr.astype(dt))
    A = mc._rows(W, sL, dt)
    lm, am = mc._metric(A)
    acc = (np.abs(lm / lr - dt(1)) <= dt(np.float32(ltol))).all(axis=1) & (np.abs(am - ar) <= dt(np.float32(angle_tol))).all(axis=1)
    assert int(acc.sum()) == out["n_mappings"] or dt is not np.float64
    use = np.flatnonzero(acc)[:mc.MAX_MAPPINGS]
    kinds, counts = np.unique(tr, return_counts=True)
    ptype = kinds[np.argmin(counts)]
    p = int(np.flatnonzero(tr == ptype)[0])
    pivots = np.flatnonzero(ts == ptype)
    xs, xr = sc.reduced_coordinates(sample["frac"], Ts).astype(dt), sc.reduced_coordinates(ref["frac"], Tr).astype(dt)
    out.update(Lr=Lr, sL=sL, xs=xs, xr=xr, p=p)
    same = tr[:, None] == ts[None, :]
    Gr = mc._gram(Lr.astype(dt))
    fn = dt(n)
    chunk = max(1, 2 ** 19 // (n * n))
    best_key = None
    marked = 0
    with np.errstate(invalid="ignore"):
        for w in use:
            Minv = np.round(np.linalg.inv(W[w].astype(np.float64))).astype(np.int64)
            G = dt(0.5) * (mc._gram(A[w]) + Gr)
            xm = mc._mapped(xs, Minv, dt)
            for j0 in range(0, len(pivots), chunk):
                J = pivots[j0:j0 + chunk]
                t = xm[J] - xr[p][None, :]
                dl = []
                for comp in range(3):
                    y = xm[None, :, comp] - t[:, comp, None]
                    dcomp = y[:, None, :] - xr[None, :, comp, None]
                    dcomp -= np.rint(dcomp)
                    dl.append(dcomp)
                uu = [(dl[0] * G[0, k] + dl[1] * G[1, k]) + dl[2] * G[2, k] for k in range(3)]
                q = (uu[0] * dl[0] + uu[1] * dl[1]) + uu[2] * dl[2]      # [J,k,i]
                del uu
                seen = np.where(np.broadcast_to(same[None], q.shape) & ~np.isnan(q), q, np.inf)
                bi = seen.argmin(axis=2)
                best = np.take_along_axis(seen, bi[..., None], axis=2)[..., 0]
                fails = ~(best <= c2)
                alive = ~fails.any(axis=1)
                dup = mc._dup_before(bi).any(axis=1)
                if dt is np.float64:
                    first = np.where(fails.any(axis=1), fails.argmax(axis=1), n)
                    decides = np.arange(n)[None, :] <= first[:, None]
                    r1 = np.sqrt(best)
                    if np.isfinite(r1[decides]).any():
                        out["pair_margin"] = min(out["pair_margin"], float(np.nanmin(np.abs(r1[decides] - c)) / c))
                    if n > 1 and alive.any():  # (which partner is nearest decides whether an alive candidate collides)
                        rest = seen[alive].copy()
                        np.put_along_axis(rest, bi[alive][..., None], np.inf, axis=2)
                        second = np.sqrt(rest.min(axis=2))
                        if np.isfinite(second).any():
                            out["gap_margin"] = min(out["gap_margin"], float(np.nanmin(second - r1[alive]) / c))
                out["n_survivors"] += int(alive.sum())
                for jj in np.flatnonzero(alive):
                    collided = bool(dup[jj])
                    if collided:
                        marked += 1
                        if marked > max_assign:
                            continue
                        out["n_assigned"] += 1
                        got = solve(q[jj], same)
                        if got is None:
                            continue
                        perm, length = got
                        out["longest_path"] = max(out["longest_path"], length)
                    else:
                        perm = bi[jj]
                    D = np.stack([dcomp[jj][np.arange(n), perm] for dcomp in dl], axis=-1)[None]
                    e = D - (mc._seq_sum(D) / fn)[:, None, :]
                    qe = mc._norm2(G, e)
                    rms = (np.sqrt(mc._seq_sum(qe) / fn) / ell)[0]
                    if dt is np.float64:
                        out["rms_margin"] = min(out["rms_margin"], abs(float(rms) - stol) / stol)
                    if not rms <= dt(np.float32(stol)):
                        continue
                    out["counting"].append((int(idx[w]), int(J[jj]), float(rms)))
                    key = (float(rms), int(idx[w]), int(J[jj]))
                    if best_key is None or key < best_key:
                        best_key = key
                        out.update(rms=float(rms), max_dist=float(np.sqrt(qe.max())), mapping=int(idx[w]), anchor=int(J[jj]),
                                   perm=np.array(perm), t=t[jj].copy(), collided=collided,
                                   cost=np.array(q[jj], dtype=np.float64), c2=float(c2))
    if marked > max_assign:
        out["flags"] |= MANY_ASSIGNMENTS
    out["matched"] = int(best_key is not None)
    if dt is np.float64 and out["matched"] and out["collided"]:
        mine = float(out["cost"][np.arange(n), out["perm"]].sum())
        out["assign_cost"] = mine
        out["assign_gap"] = (second_best(out["cost"], same, out["perm"]) - mine) / out["c2"]
    return out


# ------------------------------------------------------------------------------------------ the cases
AXIS = np.array([0.8, 0.5, 0.33]) / np.linalg.norm([0.8, 0.5, 0.33])


def _ell(L, n):
    return (abs(np.linalg.det(np.asarray(L, dtype=np.float64))) / n) ** (1 / 3)


def collide(struct, ia, ib, sample=None, axis=AXIS):
    """(reference, sample) from `struct` = (L, types, frac): reference atom ib is put 0.8 c from atom ia along `axis`
    (c = 0.3 l); in the sample (`sample` or the structure itself) ib lies 0.45 c in front of ia's site and ia 0.65 c
    behind it and 1.1 c to the side: both sites are nearest to sample atom ib (0.45 c and 0.35 c), the assignment
    ia -> ia, ib -> ib costs 1.755 c^2 against 3.515 c^2 for the exchange, and the image inverted through ia's site,
    which would pair without a collision, fails the prefilter (1.11 c)."""
    L, types, frac = struct
    L = np.asarray(L, dtype=np.float64)
    assert types[ia] == types[ib]
    c = 0.3 * _ell(L, len(types))
    side = np.cross(axis, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    inv = np.linalg.inv(L)
    ref = np.array(frac, dtype=np.float64)
    ref[ib] = ref[ia] + (0.8 * c * axis) @ inv
    smp = np.array(frac if sample is None else sample[2], dtype=np.float64)
    smp[ia] = ref[ia] + (-0.65 * c * axis + 1.1 * c * side) @ inv
    smp[ib] = ref[ia] + (0.45 * c * axis) @ inv
    return (L, types, np.mod(ref, 1.0)), (L, types, np.mod(smp, 1.0))


def _last_pair(struct):
    """(ia, ib): the last atom of the most common species and its nearest atom of that species."""
    L, types, frac = struct
    kinds, counts = np.unique(types, return_counts=True)
    ia = int(np.flatnonzero(types == kinds[np.argmax(counts)])[-1])
    d = frac - frac[ia]
    d = (d - np.rint(d)) @ np.asarray(L, dtype=np.float64)
    dist = np.where((types == types[ia]) & (np.arange(len(types)) != ia), np.linalg.norm(d, axis=1), np.inf)
    return ia, int(np.argmin(dist))


THREE = (np.diag([10.0, 4.3, 3.7]), np.array([11, 17, 17]))


@functools.lru_cache(maxsize=None)
def _build():
    base = sc._base_structures()
    cases = []

    def add(name, ref, sample, matched, nearest_matched=0, flags=0):
        cases.append(dict(name=name, ref=mc._structure(*ref), sample=mc._structure(*sample), matched=matched,
                          nearest_matched=nearest_matched, flags=flags))

    three_ref = (*THREE, np.array([[.1, .2, .3], [.40, .5, .5], [.50, .5, .5]]))
    add("three", three_ref, (*THREE, np.array([[.1, .2, .3], [.33, .5, .5], [.455, .5, .5]])), 1)
    for name in ("rutile", "rocksalt8"):
        ref, smp = collide(base[name], *_last_pair(base[name]))
        add(f"{name}_collided", ref, smp, 1)
    L4 = cc.cell(6.1, 5.2, 4.4, 90, 90, 90)
    four = (L4, np.array([11, 17, 17, 35]), np.array([[.1, .2, .3], [.5, .5, .5], [.7, .6, .4], [.3, .8, .75]]))
    add("blocks_of_one", *collide(four, 1, 2), 1)
    for k, (name, reps, skip) in enumerate((("sc_63", (4, 4, 4), True), ("sc_64", (4, 4, 4), False),
                                            ("sc_65", (4, 4, 4), False), ("sc_256", (2, 8, 16), False))):
        s = sc._supercell_sc(3.0, reps, skip_first=skip)
        if name == "sc_65":
            s = (s[0], np.append(s[1], 8), np.vstack([s[2], [[.125, .125, .125]]]))
        moved, _ = mc.displaced(s, 0.05, 300 + k)
        add(f"{name}_collided", *collide(s, *_last_pair(s), sample=moved), 1)
    # a chain of four sites 0.5 c apart, the sample 0.3 c further along: sites 2..4 are nearest to the atom before
    # their own, site 1 and site 2 collide, and the path of site 2 places sites 3 and 4 again
    Lc = np.diag([9.0, 5.0, 4.5])
    c = 0.3 * _ell(Lc, 5)
    at = np.array([2.0, 2.2, 1.9])
    chain = np.array([at + k * 0.5 * c * AXIS for k in range(4)])
    types = np.array([11, 17, 17, 17, 17])
    add("chain", (Lc, types, np.vstack([[.1, .2, .3], chain @ np.linalg.inv(Lc)])),
        (Lc, types, np.vstack([[.1, .2, .3], (chain + 0.3 * c * AXIS) @ np.linalg.inv(Lc)])), 1)
    # a cubic cell whose 16 operations that keep the x axis through the centre all carry the collided pair onto itself
    Ls = np.diag([4.0, 4.0, 4.0])
    ex = np.array([1.0, 0.0, 0.0])
    sym = (Ls, np.array([11, 17, 17]), np.array([[0, 0, 0], [.5, .5, .5], [.5, .5, .5]], dtype=np.float64))
    ref, smp = collide(sym, 1, 2, axis=ex)
    shift = (0.4 * 0.3 * _ell(Ls, 3) * ex) @ np.linalg.inv(Ls)  # (the pair's midpoint goes to the centre)
    ref[2][1:] -= shift
    smp[2][1:] -= shift
    add("symmetric16", ref, smp, 1)
    # the same pair in every cell of a 2 x 2 x 2 supercell, one species: more collided candidates than MAX_ASSIGN
    def tiled(f):
        return np.array([(f[k] + [a, b, cz]) / 2 for a in range(2) for b in range(2) for cz in range(2) for k in (1, 2)])
    big = (2 * Ls, np.full(16, 17))
    c16 = 0.3 * _ell(2 * Ls, 16) / 4.0  # (in fractions of the small cell)
    mid = np.array([.5, .5, .5])
    rf = np.array([mid, mid - 0.45 * c16 * ex, mid + 0.45 * c16 * ex])
    sf = np.array([mid, mid - 1.10 * c16 * ex, mid + 0.05 * c16 * ex])
    add("many", (*big, tiled(rf)), (*big, tiled(sf)), 1, flags=MANY_ASSIGNMENTS)
    # must still fail: one Ti of the collided rutile a further 1.0 A away
    ref, smp = collide(base["rutile"], *_last_pair(base["rutile"]))
    x = smp[2].copy()
    x[0] = x[0] + (np.array([0.6, -0.64, 0.48])) @ np.linalg.inv(smp[0])
    add("moved1", ref, (smp[0], smp[1], x), 0)
    # a NaN coordinate in the atom that would resolve the collision
    cases.append(dict(name="nan", ref=mc._structure(*three_ref), matched=0, nearest_matched=0, flags=0,
                      sample=dict(lattice=np.asarray(THREE[0], dtype=np.float32), types=THREE[1].astype(np.int64),
                                  frac=np.array([[.1, .2, .3], [.455, .5, .5], [np.nan, .5, .5]], dtype=np.float32))))
    return cases


def cases():
    return _build()


@functools.lru_cache(maxsize=None)
def reference(dtype_name="float64"):
    """The records of cases() in float32 or float64, computed once (shared; do not modify)."""
    dt = np.float32 if dtype_name == "float32" else np.float64
    return [restate_assign(c["sample"], c["ref"], dt, g) for g, c in enumerate(cases())]


def float32_error():
    """The largest |float32 - float64| over cases() and rms, max_dist, scale: the restatement's own error."""
    return max(abs(a[f] - b[f]) for a, b in zip(reference("float32"), reference("float64")) for f in mc.FLOAT_FIELDS)
