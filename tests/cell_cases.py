"""Shared inputs of the lattice-system tests (chemeleon_amd.cell, csrc/cell.hip) and the float64 numpy restatement
of the definition in include/chemeleon_hip.h at chm_cell_*:

  * `niggli(L)`: the Krivy-Gruber reduction with an epsilon of 1e-5 V^(2/3) on the squared-length scale, capped
    at 100 passes and at entries of T of 32 767, Lr = T L with T integer, det T = +1; steps A5-A7 take the whole
    multiple at once. Float64, every dot product summed in index order.
  * `deviations(Lr)` / `counts(accepted)`: every W with entries in {-1, 0, 1} and |det W| = 1, its largest
    row-length and inter-row-angle deviation from Lr's, and the counts (n, n2, n3, n4, n6) of an accepted set.
  * `classify(L, symprec, angle_tolerance, require)`: the signature table and the halving rule -> one record.

The search is defined on the reduced lattice as stored (rounded to float32), with the tolerances as float32
values, so that the device and this file decide about the same numbers; what is left to differ is the float32
arithmetic of the candidate's lengths and angles, which the margin condition of tests/test_cell_cases.py keeps
away from every decision.

Cases: the seven systems in conventional cells, primitive cells of the centred lattices, both rhombohedral
settings, each also under seeded unimodular basis changes (six shears of up to +-2 composed) and rotations, a
near-cubic cell inside the tolerances, cell(4, 4.08, 4.16, 90, 90, 90) which needs one halving, a zero-volume
cell, a NaN cell and the exactly cubic cell, where every comparison of the reduction ties.

No case ends AMBIGUOUS: the reference found none that also keeps the margin condition. A non-group at one level comes from a chain (a ~ b and b ~ c
inside the tolerance, a ~ c outside), which lasts over less than a factor of two of the tolerance, while the five
levels span a factor of sixteen; find_ambiguous() below searched 3 000 seeded perturbations of cubic, hexagonal
and rhombohedral metrics with chains on several scales and every one matched a holohedry at some level. The
flag's code path on the device is the same branch as a halving (the level's tuple is not in the table), which
one_halving exercises.
"""

import functools
import math

import numpy as np

SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "rhombohedral", "hexagonal", "cubic")
SIGNATURES = {(2, 0, 0, 0, 0): 0, (4, 1, 0, 0, 0): 1, (8, 3, 0, 0, 0): 2, (16, 5, 0, 2, 0): 3, (12, 3, 2, 0, 0): 4,
              (24, 7, 2, 0, 2): 5, (48, 9, 8, 6, 0): 6}
AMBIGUOUS, MISMATCH, NOT_REDUCED, DEGENERATE, NONFINITE = 1, 2, 4, 8, 16
SYMPREC, ANGLE_TOLERANCE = 0.1, 10.0
MAX_HALVINGS, MAX_PASSES, MAX_ENTRY = 4, 100, 32767
NIGGLI_EPS = 1.0e-5
MARGIN = 1.0e-3  # every candidate is at least MARGIN * tolerance away from the tolerance (test_cell_cases.py)


# ------------------------------------------------------------------------------------------ float64 restatement
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) + \
        m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])


def _rows(T, L):
    """T L in float64, each entry (t0 l0 + t1 l1) + t2 l2."""
    return [[(float(T[i][0]) * L[0][k] + float(T[i][1]) * L[1][k]) + float(T[i][2]) * L[2][k] for k in range(3)]
            for i in range(3)]


def _sign(v, eps):
    return 0 if abs(v) < eps else (1 if v > 0 else -1)


def niggli(lattice):
    """(T [3,3] int, passes, finished?) of the reduction of a float lattice with volume > 0. The rows are
    recomputed from T and the input in every pass, so nothing drifts."""
    L = [[float(v) for v in row] for row in np.asarray(lattice, dtype=np.float64).reshape(3, 3)]
    T = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    eps = NIGGLI_EPS * float(np.cbrt(abs(_det3(L)))) ** 2

    def neg(r):
        return [-v for v in r]

    def add_rows(T, i, j, k):  # row i += k row j; False (T unchanged) beyond the cap of T's entries
        if not abs(k) <= MAX_ENTRY:
            return False
        r = [a + int(k) * b for a, b in zip(T[i], T[j])]
        if max(abs(v) for v in r) > MAX_ENTRY:
            return False
        T[i] = r
        return True

    for passes in range(1, MAX_PASSES + 1):
        R = _rows(T, L)
        A, B, C = _dot(R[0], R[0]), _dot(R[1], R[1]), _dot(R[2], R[2])
        E, N, Y = 2.0 * _dot(R[1], R[2]), 2.0 * _dot(R[0], R[2]), 2.0 * _dot(R[0], R[1])
        if A > B + eps or (abs(A - B) < eps and abs(E) > abs(N) + eps):  # A1: a <-> b
            T = [neg(T[1]), neg(T[0]), neg(T[2])]
            A, B, E, N = B, A, N, E
        if B > C + eps or (abs(B - C) < eps and abs(N) > abs(Y) + eps):  # A2: b <-> c
            T = [neg(T[0]), neg(T[2]), neg(T[1])]
            continue
        l, m, n = _sign(E, eps), _sign(N, eps), _sign(Y, eps)
        if l * m * n == 1:  # A3: all angles acute
            i, j, k = (-1 if l == -1 else 1), (-1 if m == -1 else 1), (-1 if n == -1 else 1)
        else:  # A4: all angles obtuse or right
            i, j, k = (-1 if l == 1 else 1), (-1 if m == 1 else 1), (-1 if n == 1 else 1)
            if i * j * k == -1:
                if n == 0:
                    k = -1
                elif m == 0:
                    j = -1
                elif l == 0:
                    i = -1
        T = [[i * v for v in T[0]], [j * v for v in T[1]], [k * v for v in T[2]]]
        E, N, Y = (j * k) * E, (i * k) * N, (i * j) * Y
        # A5-A7: the whole multiple at once where the off-diagonal term exceeds the diagonal one, the unit step of
        # the published rules on the boundary cases
        step = None
        if abs(E) > B + eps:  # A5
            step = (2, 1, -float(np.rint(E / (2.0 * B))))
        elif (abs(E - B) < eps and 2.0 * N < Y - eps) or (abs(E + B) < eps and Y < -eps):
            step = (2, 1, -1.0 if E > 0 else 1.0)
        elif abs(N) > A + eps:  # A6
            step = (2, 0, -float(np.rint(N / (2.0 * A))))
        elif (abs(N - A) < eps and 2.0 * E < Y - eps) or (abs(N + A) < eps and Y < -eps):
            step = (2, 0, -1.0 if N > 0 else 1.0)
        elif abs(Y) > A + eps:  # A7
            step = (1, 0, -float(np.rint(Y / (2.0 * A))))
        elif (abs(Y - A) < eps and 2.0 * E < N - eps) or (abs(Y + A) < eps and N < -eps):
            step = (1, 0, -1.0 if Y > 0 else 1.0)
        if step is not None:
            if not add_rows(T, *step):
                return np.array(T, dtype=np.int64), passes, False
            continue
        s = E + N + Y + A + B
        if s < -eps or (abs(s) < eps and 2.0 * (A + N) + Y > eps):  # A8
            if not (add_rows(T, 2, 0, 1.0) and add_rows(T, 2, 1, 1.0)):
                return np.array(T, dtype=np.int64), passes, False
            continue
        return np.array(T, dtype=np.int64), passes, True
    return np.array(T, dtype=np.int64), MAX_PASSES, False


@functools.lru_cache(maxsize=None)
def candidates():
    """(W [M,3,3] int64, det [M], trace [M]) of the M = 6960 unimodular matrices with entries in {-1, 0, 1}, in
    the order of the index whose base-3 digits (least significant first) are the entries + 1, row by row."""
    idx = np.arange(3 ** 9)
    W = np.stack([(idx // 3 ** q) % 3 - 1 for q in range(9)], axis=1).reshape(-1, 3, 3).astype(np.int64)
    det = (W[:, 0, 0] * (W[:, 1, 1] * W[:, 2, 2] - W[:, 1, 2] * W[:, 2, 1])
           - W[:, 0, 1] * (W[:, 1, 0] * W[:, 2, 2] - W[:, 1, 2] * W[:, 2, 0])
           + W[:, 0, 2] * (W[:, 1, 0] * W[:, 2, 1] - W[:, 1, 1] * W[:, 2, 0]))
    keep = np.abs(det) == 1
    return W[keep], det[keep], np.trace(W[keep], axis1=1, axis2=2)


def lengths_angles(L):
    """(lengths [...,3], angles [...,3] = alpha (rows 1-2), beta (rows 0-2), gamma (rows 0-1) in degrees)."""
    L = np.asarray(L, dtype=np.float64)
    lens = np.sqrt((L * L).sum(-1))
    out = []
    for i, j in ((1, 2), (0, 2), (0, 1)):
        cs = (L[..., i, :] * L[..., j, :]).sum(-1) / (lens[..., i] * lens[..., j])
        out.append(np.degrees(np.arccos(np.clip(cs, -1.0, 1.0))))
    return lens, np.stack(out, -1)


def deviations(Lr):
    """Per candidate the largest |length - Lr's| over the rows (A) and the largest |angle - Lr's| (degrees)."""
    W, _, _ = candidates()
    lens0, ang0 = lengths_angles(Lr)
    lens, ang = lengths_angles(W.astype(np.float64) @ np.asarray(Lr, dtype=np.float64))
    return np.abs(lens - lens0).max(-1), np.abs(ang - ang0).max(-1)


def counts(accepted):
    _, det, tr = candidates()
    rot = accepted & (det == 1)
    return (int(accepted.sum()), int((rot & (tr == -1)).sum()), int((rot & (tr == 0)).sum()),
            int((rot & (tr == 1)).sum()), int((rot & (tr == 2)).sum()))


def classify(lattice, symprec=SYMPREC, angle_tolerance=ANGLE_TOLERANCE, require=-1):
    """The record of one float32 lattice as a dict: code, counts (n, n2, n3, n4, n6), halvings, flags, transform,
    lattice (the reduced cell, float32), lengths, angles, volume (float64 of that cell), passes, and margin: the
    smallest distance of any candidate from the acceptance boundary over the levels visited, in units of the
    level's tolerance (inf where no search ran)."""
    L32 = np.asarray(lattice, dtype=np.float32).reshape(3, 3)
    L = L32.astype(np.float64)
    sp, at = float(np.float32(symprec)), float(np.float32(angle_tolerance))
    out = dict(code=-1, counts=(0, 0, 0, 0, 0), halvings=0, flags=0, transform=np.eye(3, dtype=np.int64), passes=0,
               margin=math.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        vol = abs(_det3(L.tolist()))
        if not np.all(np.isfinite(L)):
            out["flags"] = NONFINITE
        elif not vol > 0:
            out["flags"] = DEGENERATE
        if out["flags"]:
            lens, ang = lengths_angles(L)
            d = lens[[1, 0, 0]] * lens[[2, 2, 1]]
            ang = np.where(d > 0, ang, 90.0)  # (a zero row: the screen's convention)
            out.update(lattice=L32, lengths=lens, angles=ang, volume=vol)
            if require >= 0:
                out["flags"] |= MISMATCH
            return out
    T, passes, done = niggli(L)
    Lr32 = np.array(_rows(T.tolist(), L.tolist()), dtype=np.float64).astype(np.float32)
    Lr = Lr32.astype(np.float64)
    lens, ang = lengths_angles(Lr)
    out.update(transform=T, passes=passes, lattice=Lr32, lengths=lens, angles=ang, volume=abs(_det3(Lr.tolist())))
    if not done:  # (the search means something on a reduced cell only: no system)
        out["flags"] |= NOT_REDUCED
        if require >= 0:
            out["flags"] |= MISMATCH
        return out
    dl, da = deviations(Lr)
    for h in range(MAX_HALVINGS + 1):
        tl, ta = sp * 0.5 ** h, at * 0.5 ** h
        out["margin"] = min(out["margin"], float(np.abs(dl - tl).min() / tl), float(np.abs(da - ta).min() / ta))
        c = counts((dl <= tl) & (da <= ta))
        out.update(counts=c, halvings=h)
        if c in SIGNATURES:
            out["code"] = SIGNATURES[c]
            break
    else:
        out["flags"] |= AMBIGUOUS
    if require >= 0 and out["code"] != require:
        out["flags"] |= MISMATCH
    return out


# ------------------------------------------------------------------------------------------ the cases
def cell(a, b, c, alpha, beta, gamma) -> np.ndarray:
    """Row-vector cell [3,3] (float64) of the given lengths and angles (degrees), a along x, b in the xy plane."""
    al, be, ga = (math.radians(v) for v in (alpha, beta, gamma))
    cx = math.cos(be)
    cy = (math.cos(al) - math.cos(be) * math.cos(ga)) / math.sin(ga)
    cz2 = 1.0 - cx * cx - cy * cy
    assert cz2 > 0, "not a cell"
    L = np.array([[a, 0, 0], [b * math.cos(ga), b * math.sin(ga), 0], [c * cx, c * cy, c * math.sqrt(cz2)]])
    L[np.abs(L) < 1e-15] = 0.0
    return L


def rotation(rng) -> np.ndarray:
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def unimodular(rng) -> np.ndarray:
    """Six elementary shears (row i += k row j, k in +-1, +-2) composed: an integer matrix of determinant +1."""
    U = np.eye(3, dtype=np.int64)
    for _ in range(6):
        i, j = rng.choice(3, size=2, replace=False)
        S = np.eye(3, dtype=np.int64)
        S[i, j] = rng.choice([-2, -1, 1, 2])
        U = S @ U
    return U


def _base_cells():
    """(name, system code, lattice float64, tie_free): tie_free marks cells whose reduced cell is unique, so the
    reduced angles are comparable between implementations."""
    fcc = lambda a: 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0.0]])  # noqa: E731
    body = lambda a, b, c: 0.5 * np.array([[-a, b, c], [a, -b, c], [a, b, -c]])  # noqa: E731
    mono = cell(4.0, 5.3, 6.7, 90, 104, 90)
    return [
        ("cubic", 6, cell(4, 4, 4, 90, 90, 90), False),
        ("tetragonal", 3, cell(4, 4, 6.1, 90, 90, 90), False),
        ("orthorhombic", 2, cell(4, 5.2, 6.7, 90, 90, 90), True),
        ("hexagonal", 5, cell(3.2, 3.2, 5.2, 90, 90, 120), False),
        ("rhombohedral_acute", 4, cell(5, 5, 5, 72, 72, 72), False),
        ("rhombohedral_obtuse", 4, cell(5, 5, 5, 105, 105, 105), False),
        ("monoclinic", 1, mono, True),
        ("triclinic", 0, cell(4.0, 5.3, 6.7, 78, 97, 109), True),
        ("fcc_primitive", 6, fcc(5.6), False),
        ("bcc_primitive", 6, body(4.4, 4.4, 4.4), False),
        ("bct_primitive", 3, body(4.0, 4.0, 7.0), False),
        ("ortho_C_primitive", 2, np.array([[2.0, 3.1, 0], [-2.0, 3.1, 0], [0, 0, 7.3]]), False),
        ("ortho_F_primitive", 2, 0.5 * np.array([[0, 7.0, 9.4], [5.0, 0, 9.4], [5.0, 7.0, 0]]), True),
        ("ortho_I_primitive", 2, body(4.0, 5.6, 7.4), False),
        ("mono_C_primitive", 1, np.stack([0.5 * (mono[0] + mono[1]), 0.5 * (mono[1] - mono[0]), mono[2]]), False),
    ]


def find_ambiguous(trials=3000, seed=7):
    """A seeded search for a cell whose tolerant set is a non-group at every halving level and that keeps twice
    the margin (a case of the GPU test must); None if none is found."""
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        a = 4.0 + rng.random()
        d = 10.0 ** rng.uniform(-3.0, -0.7, size=2)
        e = 10.0 ** rng.uniform(-1.0, 1.0, size=3) * rng.choice([-1, 1], size=3)
        base = rng.choice([90.0, 60.0, 120.0, 109.4712206])
        try:
            L = cell(a, a + d[0], a + d[0] + d[1], base + e[0], base + e[1], base + e[2]).astype(np.float32)
        except (AssertionError, ValueError):
            continue
        r = classify(L)
        if r["flags"] == AMBIGUOUS and r["margin"] >= 2 * MARGIN:
            return L
    return None


AMBIGUOUS_CELL = None  # (find_ambiguous() returned None: see the module's docstring)


@functools.lru_cache(maxsize=None)
def cases():
    """A list of dicts: name, lattice [3,3] float32, system (the known code; -1 where none is defined), tie_free,
    family (the base cell's name: its members must all get the same system)."""
    out = []

    def add(name, L, system, tie_free, family=None):
        out.append(dict(name=name, lattice=np.asarray(L, dtype=np.float32).reshape(3, 3), system=system,
                        tie_free=tie_free, family=family or name))

    rng = np.random.default_rng(20261020)
    for name, code, L, tie_free in _base_cells():
        add(name, L, code, tie_free)
        for v in range(3):
            add(f"{name}_u{v}", unimodular(rng) @ L @ rotation(rng), code, tie_free, family=name)
    add("near_cubic", cell(4.0, 4.02, 4.03, 90.5, 89.2, 90.8) @ rotation(rng), 6, False)
    add("one_halving", cell(4, 4.08, 4.16, 90, 90, 90), 2, True)
    # strongly sheared cells: c += 150 a and b -= 1000 a + 37 c (one pass each with whole multiples), and a shear
    # beyond the cap of T's entries, which stays NOT_REDUCED and gets no system
    add("cubic_shear150", [[4.0, 0, 0], [0, 4.0, 0], [600.0, 0, 4.0]], 6, False, family="cubic")
    tri = cell(4.0, 5.3, 6.7, 78, 97, 109)
    add("triclinic_shear1000", np.stack([tri[0], tri[1] - 1000 * tri[0] - 37 * tri[2], tri[2]]), 0, False,
        family="triclinic")
    add("not_reduced", [[4.0, 0, 0], [0, 4.0, 0], [400000.0, 0, 4.0]], -1, False)
    if AMBIGUOUS_CELL is not None:
        add("ambiguous", AMBIGUOUS_CELL, -1, False)
    add("zero_volume", [[4.0, 0, 0], [0, 5.0, 0], [4.0, 5.0, 0]], -1, False)
    add("nan", [[4.0, 0, 0], [0, float("nan"), 0], [0, 0, 5.0]], -1, False)
    return out


@functools.lru_cache(maxsize=None)
def reference(require=-1):
    """The float64 records of cases(), computed once per `require` code (shared; do not modify)."""
    return [classify(c["lattice"], SYMPREC, ANGLE_TOLERANCE, require) for c in cases()]


def batch(B):
    """The indices into cases() of a batch of B crystals: the special cases first (so the smallest batch holds a
    flagged crystal), then the rest in order, cycling."""
    cs = cases()
    first = [k for name in ("cubic", "nan", "one_halving", "zero_volume", "near_cubic", "not_reduced",
                            "cubic_shear150", "triclinic_shear1000")
             for k, c in enumerate(cs) if c["name"] == name]
    order = first + [k for k in range(len(cs)) if k not in first]
    return [order[k % len(order)] for k in range(B)]
