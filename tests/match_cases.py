"""Shared inputs of the structure-matching tests (chemeleon_amd.match, csrc/match.hip) and the numpy restatement of
the definition in include/chemeleon_hip.h at chm_match_*, parameterised by dtype:

  * `restate(sample, ref, np.float64)`: the definition in float64, which also reports the margins: how far every
    length / angle test of the lattice mappings, every pair distance that decides a pairing and every gap between a
    reference atom's nearest and second-nearest partner stay from their bounds.
  * `restate(sample, ref, np.float32)`: the same statements with every product and sum one rounded float32
    operation in the header's order, as the device computes them.

Both take T (hence the reduced cells, rounded to float32 once) from tests/cell_cases.niggli, the reduced coordinates
x' = frac(x adj(T)) from tests/symmetry_cases.reduced_coordinates, and the scale s and l = cbrt(V_r / n) from
float64 rounded to float32 once: what is left to differ between the two is the per-candidate arithmetic.

Integer fields that must agree between the two (and with the device): matched, flags, n_mappings, n_candidates,
n_survivors, ref. The winner (mapping, anchor) is not among them: a symmetric crystal has many candidates with equal
rms up to rounding, so it is held to the rule of tests/test_gpu_match.py (equal where the best is clear, else any
candidate whose float64 rms is within the gate of the best).

Cases (cases()): every reference of REFERENCES against samples derived from it that must match (a seeded rotation,
unimodular basis change, permutation and origin shift at once; scale 0.9 and 1.1; displacements of 0.05 A; a 5%
uniaxial strain; the inverted, i.e. mirror-image, quartz) and that must not (a uniaxial strain of 30%, taken as a
compression to 0.7: with scaling always on, a stretch to 1.3 changes no length by more than 19.1%, inside ltol;
a cell with gamma off by 8 degrees; one atom moved by 1.0 A; rutile with one Ti and one O exchanged), the flag
cases, and simple-cubic supercells of 63, 64, 65 and 256 atoms against themselves displaced.
"""

import functools
import math

import numpy as np

from tests import cell_cases as cc
from tests import symmetry_cases as sc

NO_REFERENCE, NO_LATTICE, SIZE, COMPOSITION, THIN, MANY_MAPPINGS = 1, 2, 4, 8, 16, 32
LTOL, STOL, ANGLE_TOL = 0.2, 0.3, 5.0
MAX_MAPPINGS = 256
MARGIN = 1.0e-3
INT_FIELDS = ("matched", "flags", "n_mappings", "n_candidates", "n_survivors", "ref")
FLOAT_FIELDS = ("rms", "max_dist", "scale")
DEG = 57.29577951308232


# ------------------------------------------------------------------------------------------ the restatement
@functools.lru_cache(maxsize=None)
def _candidates():
    """(index [M], W [M,3,3] int64, det [M]) of the unimodular candidates in ascending index order."""
    W, det, _ = cc.candidates()
    idx = np.array([sc.candidate_index(w) for w in W])
    assert np.all(np.diff(idx) > 0)
    return idx, W, det


def reduced(lattice):
    """(T, the reduced cell as float32) of a float32 lattice, or None where its cell record carries no reduced cell
    (non-finite, zero volume, or a reduction that did not finish)."""
    L32 = np.asarray(lattice, dtype=np.float32).reshape(3, 3)
    L = L32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if not np.all(np.isfinite(L)) or not abs(cc._det3(L.tolist())) > 0:
            return None
    T, _, done = cc.niggli(L)
    if not done:
        return None
    return T, np.array(cc._rows(T.tolist(), L.tolist()), dtype=np.float64).astype(np.float32)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _rows(W, A, dt):
    """W A per candidate, entries (w0 a0 + w1 a1) + w2 a2, each operation rounded in dt. W [...,3,3] -> [...,3,3]."""
    W = W.astype(dt)
    return np.stack([np.stack([(W[..., i, 0] * A[0, k] + W[..., i, 1] * A[1, k]) + W[..., i, 2] * A[2, k]
                               for k in range(3)], axis=-1) for i in range(3)], axis=-2)


def _metric(A):
    """(lengths [...,3], angles [...,3] = rows 1-2, 0-2, 0-1 in degrees) in A's dtype, as the device forms them."""
    dt = A.dtype.type
    l = np.stack([np.sqrt(_dot(A[..., i, :], A[..., i, :])) for i in range(3)], axis=-1)
    ang = []
    for i, j in ((1, 2), (0, 2), (0, 1)):
        cs = np.clip(_dot(A[..., i, :], A[..., j, :]) / (l[..., i] * l[..., j]), dt(-1), dt(1))
        ang.append(np.arccos(cs) * dt(DEG))
    return l, np.stack(ang, axis=-1)


def _gram(A):
    return np.stack([np.stack([_dot(A[..., i, :], A[..., j, :]) for j in range(3)], axis=-1) for i in range(3)], axis=-2)


def _norm2(G, d):
    u = [(d[..., 0] * G[0, k] + d[..., 1] * G[1, k]) + d[..., 2] * G[2, k] for k in range(3)]
    return (u[0] * d[..., 0] + u[1] * d[..., 1]) + u[2] * d[..., 2]


def _mapped(x, Minv, dt):
    Mi = Minv.astype(dt)
    y = np.stack([(x[..., 0] * Mi[0, k] + x[..., 1] * Mi[1, k]) + x[..., 2] * Mi[2, k] for k in range(3)], axis=-1)
    f = y - np.floor(y)
    f[f >= 1] = 0
    return f


def _seq_sum(a):
    """The sum over axis 1 in index order, one rounded addition per term."""
    s = np.zeros_like(a[:, 0])
    for k in range(a.shape[1]):
        s = s + a[:, k]
    return s


def _dup_before(bi):
    """[J,n] bool: entry k equals an entry k' < k of its row."""
    order = np.argsort(bi, axis=1, kind="stable")
    srt = np.take_along_axis(bi, order, axis=1)
    dup_sorted = np.zeros_like(bi, dtype=bool)
    dup_sorted[:, 1:] = srt[:, 1:] == srt[:, :-1]
    out = np.zeros_like(dup_sorted)
    np.put_along_axis(out, order, dup_sorted, axis=1)
    return out


def score(sample_x, ref_x, Lr, sL, M, t, perm, ell, dt=np.float64):
    """(rms, max_dist) of the pairing `perm` (reference atom k -> sample atom perm[k]) under mapping M and shift t:
    the header's score, recomputed from the winner alone (the check of the device's perm output)."""
    Minv = np.round(np.linalg.inv(M.astype(np.float64))).astype(np.int64)
    G = dt(0.5) * (_gram(_rows(M, sL.astype(dt), dt)) + _gram(Lr.astype(dt)))
    xm = _mapped(sample_x.astype(dt), Minv, dt)
    d = (xm[perm] - t.astype(dt)) - ref_x.astype(dt)
    d = d - np.rint(d)
    e = d - _seq_sum(d[None])[0] / dt(len(d))
    q = _norm2(G, e)
    return float(np.sqrt(_seq_sum(q[None])[0] / dt(len(d))) / dt(ell)), float(np.sqrt(q.max()))


def restate(sample, ref, dtype=np.float64, ref_index=0, ltol=LTOL, stol=STOL, angle_tol=ANGLE_TOL):
    """The record of one (sample, reference) pair as a dict: INT_FIELDS, rms, max_dist, scale, l, mapping, anchor,
    `counting` (a list of (mapping index, anchor atom, rms) of every candidate that counts), the frames (Lr, sL, xs,
    xr, p) for the checks of perm, and the margins (float64 only): lattice_margin, pair_margin, gap_margin, in units
    of the tolerance / of c. sample and ref are dicts of lattice (float32 [3,3]), types, frac (float32); ref None =
    no reference."""
    dt = dtype
    out = dict(rms=0.0, max_dist=0.0, scale=0.0, l=0.0, mapping=-1, anchor=-1, n_mappings=0, n_candidates=0,
               n_survivors=0, matched=0, flags=0, ref=ref_index if ref is not None else -1, counting=[],
               lattice_margin=math.inf, pair_margin=math.inf, gap_margin=math.inf, thin_margin=math.inf)
    if ref is None:
        out["flags"] = NO_REFERENCE
        return out
    rs, rr = reduced(sample["lattice"]), reduced(ref["lattice"])
    ts, tr = np.asarray(sample["types"], dtype=np.int64), np.asarray(ref["types"], dtype=np.int64)
    n = len(tr)
    if rs is None or rr is None:
        out["flags"] |= NO_LATTICE
    if len(ts) != n:
        out["flags"] |= SIZE
    elif sorted(ts.tolist()) != sorted(tr.tolist()):
        out["flags"] |= COMPOSITION
    if rs is not None and rr is not None:
        (Ts, Ls), (Tr, Lr) = rs, rr
        vs, vr = abs(cc._det3(Ls.astype(np.float64).tolist())), abs(cc._det3(Lr.astype(np.float64).tolist()))
        if not (0 < vs < math.inf and 0 < vr < math.inf):
            out["flags"] |= NO_LATTICE
        else:
            out["scale"] = float(np.float32(np.cbrt(vr / vs)))
            out["l"] = float(np.float32(np.cbrt(vr / n)))
    if out["flags"]:
        return out
    scale, ell = dt(np.float32(out["scale"])), dt(np.float32(out["l"]))
    c = dt(np.float32(stol)) * ell
    c2 = c * c
    d = sc.spacings(Lr, dt)
    if not dt(2) * c < min(d):
        out["flags"] = THIN
        return out
    if dt is np.float64:
        out["thin_margin"] = abs(float(min(d)) - 2 * float(c)) / (2 * float(c))
    # the lattice mappings
    idx, W, det = _candidates()
    sL = scale * Ls.astype(dt)
    lr, ar = _metric(Lr.astype(dt))
    A = _rows(W, sL, dt)
    lm, am = _metric(A)
    dev_l, dev_a = np.abs(lm / lr - dt(1)), np.abs(am - ar)
    tl, ta = dt(np.float32(ltol)), dt(np.float32(angle_tol))
    len_ok = (dev_l <= tl).all(axis=1)
    acc = len_ok & (dev_a <= ta).all(axis=1)
    if dt is np.float64:
        out["lattice_margin"] = min(float(np.abs(dev_l - tl).min() / tl), float(np.abs(dev_a[len_ok] - ta).min() / ta)
                                    if len_ok.any() else math.inf)
    out["n_mappings"] = int(acc.sum())
    if out["n_mappings"] > MAX_MAPPINGS:
        out["flags"] |= MANY_MAPPINGS
    use = np.flatnonzero(acc)[:MAX_MAPPINGS]
    # the anchors
    kinds, counts = np.unique(tr, return_counts=True)
    ptype = kinds[np.argmin(counts)]
    p = int(np.flatnonzero(tr == ptype)[0])
    pivots = np.flatnonzero(ts == ptype)
    out["n_candidates"] = len(use) * len(pivots)
    xs, xr = sc.reduced_coordinates(sample["frac"], Ts).astype(dt), sc.reduced_coordinates(ref["frac"], Tr).astype(dt)
    out.update(Lr=Lr, sL=sL, xs=xs, xr=xr, p=p)
    same = tr[:, None] == ts[None, :]  # [k, i]
    Gr = _gram(Lr.astype(dt))
    fn = dt(n)
    chunk = max(1, 2 ** 19 // (n * n))
    best_key = None
    for w in use:
        Minv = np.round(np.linalg.inv(W[w].astype(np.float64))).astype(np.int64)
        assert np.array_equal(Minv @ W[w], np.eye(3, dtype=np.int64))
        G = dt(0.5) * (_gram(A[w]) + Gr)
        xm = _mapped(xs, Minv, dt)
        for j0 in range(0, len(pivots), chunk):
            J = pivots[j0:j0 + chunk]
            t = xm[J] - xr[p][None, :]                                   # [J,3]
            dl = []                                                      # per component [J,k,i]
            for comp in range(3):
                y = xm[None, :, comp] - t[:, comp, None]                 # [J,i]
                dcomp = y[:, None, :] - xr[None, :, comp, None]
                dcomp -= np.rint(dcomp)
                dl.append(dcomp)
            u = [(dl[0] * G[0, k] + dl[1] * G[1, k]) + dl[2] * G[2, k] for k in range(3)]
            q = (u[0] * dl[0] + u[1] * dl[1]) + u[2] * dl[2]             # [J,k,i]
            del u
            q[np.broadcast_to(~same[None], q.shape)] = np.inf
            bi = q.argmin(axis=2)                                        # (the first minimum: ties to the smallest i)
            best = np.take_along_axis(q, bi[..., None], axis=2)[..., 0]  # [J,k]
            fails = ~(best <= c2) | _dup_before(bi)
            alive = ~fails.any(axis=1)
            if dt is np.float64:
                first = np.where(fails.any(axis=1), fails.argmax(axis=1), n)
                decides = np.arange(n)[None, :] <= first[:, None]
                with np.errstate(invalid="ignore"):
                    r1 = np.sqrt(best)
                    if decides.any() and np.isfinite(r1[decides]).any():
                        out["pair_margin"] = min(out["pair_margin"], float(np.abs(r1[decides] - c).min() / c))
                    if q.shape[2] > 1:
                        np.put_along_axis(q, bi[..., None], np.inf, axis=2)
                        second = np.sqrt(q.min(axis=2))
                        both = decides & (second <= c)
                        if both.any():
                            out["gap_margin"] = min(out["gap_margin"], float((second - r1)[both].min() / c))
            if not alive.any():
                continue
            out["n_survivors"] += int(alive.sum())
            Ja, bia = J[alive], bi[alive]
            D = np.stack([np.take_along_axis(dcomp[alive], bia[..., None], axis=2)[..., 0] for dcomp in dl], axis=-1)
            e = D - (_seq_sum(D) / fn)[:, None, :]
            qe = _norm2(G, e)
            rms = np.sqrt(_seq_sum(qe) / fn) / ell
            maxd = np.sqrt(qe.max(axis=1))
            for jj in np.flatnonzero(rms <= dt(np.float32(stol))):
                out["counting"].append((int(idx[w]), int(Ja[jj]), float(rms[jj])))
                key = (float(rms[jj]), int(idx[w]), int(Ja[jj]))
                if best_key is None or key < best_key:
                    best_key = key
                    out.update(rms=float(rms[jj]), max_dist=float(maxd[jj]), mapping=int(idx[w]), anchor=int(Ja[jj]),
                               perm=bia[jj].copy(), t=t[alive][jj].copy())
    out["matched"] = int(best_key is not None)
    return out


# ------------------------------------------------------------------------------------------ the cases
def _structure(L, types, frac):
    return dict(lattice=np.asarray(L, dtype=np.float32).reshape(3, 3), types=np.asarray(types, dtype=np.int64),
                frac=np.mod(np.asarray(frac, dtype=np.float32), np.float32(1)))


def displaced(struct, amplitude, seed):
    """(structure, v [n,3]): every atom moved by `amplitude` A in a seeded direction; v are the Cartesian moves."""
    L, types, frac = struct
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(np.shape(frac))
    v *= amplitude / np.linalg.norm(v, axis=1, keepdims=True)
    return (L, types, np.mod(frac + v @ np.linalg.inv(L), 1.0)), v


def expected_rms(v, struct):
    """The displacement's own rms after mean removal, in units of l = (V / n)^(1/3)."""
    L = np.asarray(struct[0], dtype=np.float64)
    e = v - v.mean(axis=0)
    return math.sqrt((e * e).sum(axis=1).mean()) / (abs(np.linalg.det(L)) / len(v)) ** (1 / 3)


def _with_gamma(L, delta):
    lens, ang = cc.lengths_angles(L)
    return cc.cell(lens[0], lens[1], lens[2], ang[0], ang[1], ang[2] + delta)


# the references whose gamma + 8 degrees is a different lattice under the definition: in an fcc-primitive or a
# hexagonal cell the same change is 4 degrees or less in another basis (a, a + b), inside angle_tol, and matches
SHEARED = ("simple_cubic", "cscl", "rocksalt8", "rutile", "p1_five")
REFERENCES = ("simple_cubic", "cscl", "rocksalt_primitive", "rocksalt8", "diamond_primitive", "rutile", "wurtzite",
              "quartz", "p1_five")


@functools.lru_cache(maxsize=None)
def _build():
    """(references: list of (name, structure dict), cases: list of dicts)."""
    base = sc._base_structures()
    tri = cc.cell(4.0, 5.3, 6.7, 78, 97, 109)
    base["p1_five"] = (tri, np.array([20, 8, 8, 6, 6]), np.array([[.05, .11, .23], [.31, .62, .17], [.55, .29, .71],
                                                                   [.83, .47, .39], [.19, .88, .64]]))
    for name, reps, skip in (("sc_63", (4, 4, 4), True), ("sc_64", (4, 4, 4), False), ("sc_256", (2, 8, 16), False)):
        base[name] = sc._supercell_sc(3.0, reps, skip_first=skip)
    L, types, frac = sc._supercell_sc(3.0, (4, 4, 4))
    base["sc_65"] = (L, np.append(types, 8), np.vstack([frac, [[.125, .125, .125]]]))
    base["thin"] = (cc.cell(4, 5.2, 0.19, 90, 90, 90), np.array([29]), np.array([[0.0, 0, 0]]))
    names = list(REFERENCES) + ["sc_63", "sc_64", "sc_65", "sc_256", "thin"]
    refs = [(name, _structure(*base[name])) for name in names]
    at = {name: k for k, name in enumerate(names)}
    cases = []

    def add(name, struct, ref, matched, flags=0, rms=None):
        cases.append(dict(name=name, sample=_structure(*struct), ref=-1 if ref is None else at[ref], matched=matched,
                          flags=flags, rms=rms))

    rng = np.random.default_rng(20261020)
    for k, name in enumerate(REFERENCES):
        L, types, frac = base[name]
        add(f"{name}_variant", sc._variant(base[name], rng), name, 1)
        add(f"{name}_scale09", (0.9 * L, types, frac), name, 1)
        add(f"{name}_scale11", (1.1 * L, types, frac), name, 1)
        moved, v = displaced(base[name], 0.05, 100 + k)
        add(f"{name}_d005", moved, name, 1, rms=expected_rms(v, base[name]))
        add(f"{name}_strain5", (L @ np.diag([1.05, 1, 1]), types, frac), name, 1)
        add(f"{name}_strain30", (L @ np.diag([0.7, 1, 1]), types, frac), name, 0)
        if name in SHEARED:
            add(f"{name}_shear8", (_with_gamma(L, 8.0), types, frac), name, 0)
        if len(types) > 1:  # (moving the only atom of a cell is an origin shift)
            u = rng.standard_normal(3)
            x = np.array(frac, dtype=np.float64)
            x[-1] = x[-1] + (u / np.linalg.norm(u)) @ np.linalg.inv(L)
            add(f"{name}_moved1", (L, types, x), name, 0)
    L, types, frac = base["quartz"]
    add("quartz_mirror", (L @ cc.rotation(rng), types, np.mod(-frac, 1.0)), "quartz", 1)
    L, types, frac = base["rutile"]
    swapped = types.copy()
    ti, ox = int(np.flatnonzero(types == 22)[0]), int(np.flatnonzero(types == 8)[0])
    swapped[ti], swapped[ox] = 8, 22
    add("rutile_exchanged", (L, swapped, frac), "rutile", 0)
    # the flags
    L, types, frac = base["cscl"]
    add("composition", (L, np.array([55, 55]), frac), "cscl", 0, COMPOSITION)
    add("size", base["rocksalt8"], "rocksalt_primitive", 0, SIZE)
    add("no_reference", base["cscl"], None, 0, NO_REFERENCE)
    add("nan_cell", ([[4.1, 0, 0], [0, float("nan"), 0], [0, 0, 4.1]], types, frac), "cscl", 0, NO_LATTICE)
    add("zero_volume", ([[4.1, 0, 0], [0, 4.1, 0], [4.1, 4.1, 0]], types, frac), "cscl", 0, NO_LATTICE)
    add("thin", base["thin"], "thin", 0, THIN)
    # sizes at the wave and block edges (N = 1 and 2 are simple_cubic and cscl above)
    for k, name in enumerate(("sc_63", "sc_64", "sc_65", "sc_256")):
        moved, v = displaced(base[name], 0.05, 200 + k)
        add(f"{name}_d005", moved, name, 1)
    return refs, cases


def references():
    return _build()[0]


def cases():
    return _build()[1]


@functools.lru_cache(maxsize=None)
def reference(dtype_name="float64"):
    """The records of cases() in float32 or float64, computed once (shared; do not modify)."""
    dt = np.float32 if dtype_name == "float32" else np.float64
    refs = references()
    return [restate(c["sample"], refs[c["ref"]][1] if c["ref"] >= 0 else None, dt, c["ref"]) for c in cases()]


def float32_error():
    """The largest |float32 - float64| over cases() and FLOAT_FIELDS: the restatement's own error."""
    return max(abs(a[f] - b[f]) for a, b in zip(reference("float32"), reference("float64")) for f in FLOAT_FIELDS)


def packed(structs):
    """(natoms, types int64 [N], frac float32 [N,3], lattices float32 [B,3,3]) of a list of structure dicts."""
    return ([len(s["types"]) for s in structs], np.concatenate([s["types"] for s in structs]),
            np.concatenate([s["frac"] for s in structs]), np.stack([s["lattice"] for s in structs]))
