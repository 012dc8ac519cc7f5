"""Shared inputs of the screening tests (chemeleon_amd.screening, csrc/screen.hip) and two numpy restatements of
what the kernel computes:

  * `reference(...)`: float64, the shortest distance by brute force over the fractional difference wrapped to
    [-0.5, 0.5] and the images -7..7 per axis, exact integer formula reduction. The yardstick of the GPU tests.
  * `two_pass_f32(...)`: the kernel's two-pass search (27 images, then the range from the plane spacings,
    capped at 4) in float32 numpy. It checks the fixtures, not the kernel: the method and the number format stay
    inside the gate on every uncapped case (tests/test_screen_cases.py).

The cases are small because the kernel's risks are boundaries, not size: one ragged batch with crystals of 1, 2,
64, 65, 256, 257 and 300 atoms (wave boundary, LDS tile boundary, tile pairs), the wrap at a cell face, coincident
atoms, cubic / triclinic / skewed cells whose image range is 1, 2 and 3 (in the last two the closest image lies
outside the 27 neighbouring cells, in the last outside the 125), one beyond the cap, one of zero volume,
one edge above max_length, and the composition cases.
"""

import functools
import math

import numpy as np

MAX_LENGTH, MIN_DISTANCE = 60.0, 0.5
TOO_LONG, TOO_CLOSE, COMPOSITION, DEGENERATE, NONFINITE = 1, 2, 4, 8, 16
MAX_RANGE = 4  # the kernel's cap of the image range per axis
BRUTE = 7      # the float64 restatement searches images -7..7
TI, O, SR = 22, 8, 38


def gate(lengths) -> float:
    """The absolute tolerance of lengths and distances: 16 * 2^-24 * (a + b + c). Each Cartesian component is
    three rounded products of a fractional value of at most 4.5 by a lattice entry."""
    return 16.0 * 2.0 ** -24 * float(np.sum(lengths))


def cell_from_parameters(a, b, c, alpha, beta, gamma, rotate_seed=None) -> np.ndarray:
    """Row-vector cell [3,3] (float32) of the given lengths and angles (degrees), rotated by a random rotation
    so that no entry is zero."""
    al, be, ga = (math.radians(v) for v in (alpha, beta, gamma))
    cx = math.cos(be)
    cy = (math.cos(al) - math.cos(be) * math.cos(ga)) / math.sin(ga)
    cz2 = 1.0 - cx * cx - cy * cy
    assert cz2 > 0, "not a cell"
    L = np.array([[a, 0, 0], [b * math.cos(ga), b * math.sin(ga), 0], [c * cx, c * cy, c * math.sqrt(cz2)]])
    if rotate_seed is not None:
        q, _ = np.linalg.qr(np.random.default_rng(rotate_seed).standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        L = L @ q
    return L.astype(np.float32)


def _random_types(rng, n, pool):
    return rng.choice(np.array(pool, dtype=np.int64), size=n)


@functools.lru_cache(maxsize=None)
def cases():
    """The ragged batch: a list of dicts (name, lattice [3,3] f32, frac [n,3] f32, types [n] int64, compare_dmin,
    formula: the crystal's own entry of the per-crystal target list)."""
    rng = np.random.default_rng(20261020)
    out = []

    def add(name, lattice, frac, types, compare_dmin=True, formula="TiO2"):
        frac = np.asarray(frac, dtype=np.float32).reshape(-1, 3)
        types = np.asarray(types, dtype=np.int64).reshape(-1)
        assert len(frac) == len(types)
        out.append(dict(name=name, lattice=np.asarray(lattice, dtype=np.float32).reshape(3, 3), frac=frac, types=types,
                        compare_dmin=compare_dmin, formula=formula))

    cubic = lambda a: np.eye(3, dtype=np.float32) * a  # noqa: E731
    add("one_atom", cubic(5.0), [[0.2, 0.4, 0.6]], [TI], formula="Ti")
    add("wrap", cubic(4.0), [[1e-6, 0.3, 0.3], [0.999999, 0.3, 0.3]], [TI, O], formula="TiO")
    add("coincident", cell_from_parameters(4, 5, 6, 80, 95, 100, 1), [[0.25, 0.5, 0.75]] * 2, [O, O], formula="O")
    add("n64_triclinic", cell_from_parameters(9, 10, 11, 70, 100, 115, 2), rng.random((64, 3)),
        _random_types(rng, 64, [TI, O]), formula="SrTiO3")
    add("n65_20deg", cell_from_parameters(12, 13, 14, 20, 75, 80, 3), rng.random((65, 3)),
        _random_types(rng, 65, [TI, O, SR]), formula="SrTiO3")
    add("n256_cubic", cubic(24.0), rng.random((256, 3)), _random_types(rng, 256, [TI, O]))
    add("n257_160deg", cell_from_parameters(22, 20, 25, 95, 160, 85, 4), rng.random((257, 3)),
        _random_types(rng, 257, [TI, O]))
    t300 = np.array([TI] * 100 + [O] * 200, dtype=np.int64)
    add("n300_triclinic", cell_from_parameters(25, 24, 26, 60, 110, 75, 5), rng.random((300, 3)), rng.permutation(t300))
    # skewed cells: row 1 sheared along row 0, so the closest image of the pair lies beyond the 27 neighbours
    add("skew_R1", [[3.0, 0, 0], [6.5, 3.0, 0], [0, 0, 10.0]], [[0.0, 0.0, 0.0], [0.45, 0.5, 0.0]], [TI, O],
        formula="TiO")
    add("skew_R2", [[3.0, 0, 0], [9.5, 3.4, 0], [0, 0, 10.0]], [[0.1, 0.2, 0.3], [0.43, 0.7, 0.3]], [TI, O],
        formula="TiO")
    add("skew_R2_rotated", cell_from_parameters(3.0, 10.09, 10.0, 90, 90, 19.69, 6),
        [[0.6, 0.9, 0.3], [0.93, 0.4, 0.3], [0.2, 0.1, 0.8]], [TI, O, O])
    add("skew_R3", [[3.0, 0, 0], [13.5, 2.0, 0], [0, 0, 10.0]], [[0.1, 0.2, 0.3], [0.2, 0.5, 0.3]], [TI, O],
        formula="TiO")
    add("beyond_cap", [[3.0, 0, 0], [16.0, 3.0, 0], [0, 0, 10.0]], [[0.0, 0.0, 0.0], [0.3, 0.5, 0.5]], [TI, O],
        compare_dmin=False, formula="TiO")
    add("zero_volume", [[4.0, 0, 0], [0, 5.0, 0], [4.0, 5.0, 0]], [[0.1, 0.1, 0.1], [0.4, 0.4, 0.2]], [TI, O],
        compare_dmin=False, formula="TiO")
    add("long_edge", [[60.5, 0, 0], [0, 5.0, 0], [0, 0, 5.0]], [[0.1, 0.1, 0.1], [0.5, 0.6, 0.5], [0.9, 0.2, 0.8]],
        [TI, O, O])
    f12 = rng.random((12, 3))
    add("Ti4O8", cubic(6.0), f12, [TI] * 4 + [O] * 8)
    add("Ti2O4", cell_from_parameters(4.6, 4.6, 3.0, 90, 90, 90, 7), rng.random((6, 3)), [O, TI, O, O, TI, O])
    add("Ti3O5", cubic(5.5), rng.random((8, 3)), [TI] * 3 + [O] * 5)
    add("Ti3O5_own_target", cubic(5.5), rng.random((8, 3)), [TI] * 3 + [O] * 5, formula="Ti3O5")
    add("class_104", cubic(5.0), [[0.1, 0.1, 0.1], [0.5, 0.5, 0.5], [0.1, 0.6, 0.6]], [TI, O, 104])
    add("Sr2Ti2O6_own_target", cubic(5.6), rng.random((10, 3)), [SR, SR, TI, TI] + [O] * 6, formula="SrTiO3")
    return out


def natoms():
    return [len(c["types"]) for c in cases()]


def batch_arrays():
    """(atom_types [N] int64, frac [N,3] f32, lattices [B,3,3] f32) of the whole batch."""
    cs = cases()
    return (np.concatenate([c["types"] for c in cs]), np.concatenate([c["frac"] for c in cs]),
            np.stack([c["lattice"] for c in cs]))


TARGET_MODES = ("none", "shared", "per_crystal")


def composition_for(mode):
    """The `composition` argument of Screen for a target mode."""
    return {"none": None, "shared": "TiO2", "per_crystal": [c["formula"] for c in cases()]}[mode]


# ------------------------------------------------------------------------------------------ float64 restatement
def clamp_types(types):
    t = np.asarray(types, dtype=np.int64)
    return np.where((t >= 0) & (t <= 103), t, 0)


def formula_units_and_reduced(types):
    cnt = np.bincount(clamp_types(types), minlength=104).astype(np.int64)
    g = 0
    for c in cnt:
        g = math.gcd(g, int(c))
    return g, cnt // g


def reduced_target(formula):
    """The reduced counts [104] of a formula string, parsed here (element symbols + optional integer counts)."""
    import re
    from chemeleon_amd.modules.schema import CHEMICAL_SYMBOLS
    cnt = np.zeros(104, dtype=np.int64)
    for sym, num in re.findall(r"([A-Z][a-z]?)(\d*)", formula):
        cnt[CHEMICAL_SYMBOLS.index(sym)] += int(num) if num else 1
    g = 0
    for c in cnt:
        g = math.gcd(g, int(c))
    return cnt // g


def cell_f64(lattice):
    L = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    lens = np.linalg.norm(L, axis=1)

    def ang(i, j):
        return math.degrees(math.acos(np.clip(np.dot(L[i], L[j]) / (lens[i] * lens[j]), -1.0, 1.0)))

    vol = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
    return L, lens, np.array([ang(1, 2), ang(0, 2), ang(0, 1)]), vol


def plane_spacings(L, vol):
    cr = [np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([vol / np.linalg.norm(c) for c in cr])


def _pair_diffs(frac, dtype):
    f = np.asarray(frac, dtype=dtype)
    i, j = np.triu_indices(len(f), k=1)
    w = f[j] - f[i]
    return i, j, (w - np.rint(w)).astype(dtype)


def _search(w, L, R, dtype):
    """min over pairs and images n_k in [-R_k, R_k] of |(w + n) L|^2 in `dtype`, each component summed over
    k = 0, 1, 2 in order -> (d2 per pair [P])."""
    best = np.full(len(w), np.inf, dtype=dtype)
    for n0 in range(-R[0], R[0] + 1):
        for n1 in range(-R[1], R[1] + 1):
            for n2 in range(-R[2], R[2] + 1):
                v = w + np.array([n0, n1, n2], dtype=dtype)
                c = (v[:, 0:1] * L[0] + v[:, 1:2] * L[1]) + v[:, 2:3] * L[2]
                d2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
                best = np.minimum(best, d2)
    return best


def _brute(w, L):
    """min over pairs and the images -BRUTE..BRUTE of |(w + n) L| in float64. Every image of every pair is
    evaluated, in the expanded form |C|^2 + 2 C.t + |t|^2 (one matrix product per chunk of pairs); the winner
    of each pair is then recomputed directly, so the expansion's cancellation (about 1e-10 A here) can only
    swap images that are that close to a tie."""
    r = np.arange(-BRUTE, BRUTE + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    t = n @ L
    t2 = (t * t).sum(1)
    best = np.inf
    for k in range(0, len(w), 8192):
        wk = w[k:k + 8192]
        c = wk @ L
        d2 = (c * c).sum(1)[:, None] + 2.0 * (c @ t.T) + t2[None, :]
        v = c + t[d2.argmin(1)]
        best = min(best, float(np.sqrt((v * v).sum(1).min())))
    return best


def image_ranges(d0, h):
    """(R [3] capped at MAX_RANGE, r [3] the uncapped bounds 0.5 + d0 / h_k, capped?)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (0.5 + d0 / h) * (1.0 + 1.0e-5)
    capped = bool(np.any(~(r < MAX_RANGE + 1)))
    R = [MAX_RANGE if not (x < MAX_RANGE + 1) else int(math.floor(x)) for x in r]
    return R, r, capped


def pair_distance_f64(lattice, frac, i, j):
    """The float64 minimum-image distance of one pair (images -7..7)."""
    L = np.asarray(lattice, dtype=np.float64)
    w = np.asarray(frac[j], dtype=np.float64) - np.asarray(frac[i], dtype=np.float64)
    w = (w - np.rint(w))[None, :]
    return float(np.sqrt(_search(w, L, [BRUTE] * 3, np.float64)[0]))


@functools.lru_cache(maxsize=None)
def geometry():
    """Per crystal, computed once: (L, lengths, angles, volume, dmin, d27, degenerate, ranges r [3])."""
    out = []
    for c in cases():
        L, lens, angles, vol = cell_f64(c["lattice"])
        n = len(c["types"])
        if n > 1:
            _, _, w = _pair_diffs(c["frac"], np.float64)
            dmin = _brute(w, L)
            d27 = float(np.sqrt(_search(w, L, [1] * 3, np.float64).min()))
        else:
            dmin = d27 = math.inf
        degenerate, r = not vol > 0, np.zeros(3)
        if n > 1 and not degenerate:
            _, r, degenerate = image_ranges(d27, plane_spacings(L, vol))
        out.append((L, lens, angles, vol, dmin, d27, degenerate, r))
    return out


@functools.lru_cache(maxsize=None)
def reference(mode="none", max_length=MAX_LENGTH, min_distance=MIN_DISTANCE):
    """The float64 records of the batch under a target mode: a list of dicts (lengths, angles, volume, dmin,
    formula_units, flags, ranges r [3] of the two-pass bound, d27: the minimum over the 27 images only)."""
    out = []
    for c, (L, lens, angles, vol, dmin, d27, degenerate, r) in zip(cases(), geometry()):
        units, red = formula_units_and_reduced(c["types"])
        flags = 0
        if lens.max() > max_length:
            flags |= TOO_LONG
        if dmin < min_distance:
            flags |= TOO_CLOSE
        if mode != "none":
            tg = reduced_target("TiO2" if mode == "shared" else c["formula"])
            if not np.array_equal(red, tg):
                flags |= COMPOSITION
        if degenerate:
            flags |= DEGENERATE
        out.append(dict(name=c["name"], lengths=lens, angles=angles, volume=vol, dmin=dmin, d27=d27, formula_units=units,
                        flags=flags, ranges=r))
    return out


# ------------------------------------------------------------------------------------------ float32 restatement
def two_pass_f32(lattice, frac):
    """The kernel's method in float32 numpy -> (lengths [3], volume, dmin, capped?)."""
    f32 = np.float32
    L = np.asarray(lattice, dtype=f32)
    lens = np.sqrt(((L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2]).astype(f32))
    cr = [np.cross(L[1], L[2]).astype(f32), np.cross(L[2], L[0]).astype(f32), np.cross(L[0], L[1]).astype(f32)]
    vol = f32(abs((L[0, 0] * cr[0][0] + L[0, 1] * cr[0][1]) + L[0, 2] * cr[0][2]))
    if len(frac) < 2:
        return lens, vol, math.inf, False
    _, _, w = _pair_diffs(frac, f32)
    d2 = _search(w, L, [1, 1, 1], f32).min()
    if not vol > 0:
        return lens, vol, float(np.sqrt(d2)), True
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.array([vol / np.sqrt((c * c).sum(dtype=f32)) for c in cr], dtype=f32)
    R, _, capped = image_ranges(np.sqrt(d2), h)
    if max(R) > 1:
        d2 = _search(w, L, [max(x, 1) for x in R], f32).min()
    return lens, vol, float(np.sqrt(d2)), capped
