"""Shared inputs of the dedup tests (chemeleon_amd.dedup, csrc/dedup.hip) and plain restatements of what the
kernels compute, no device:

  * `fingerprint_f64(...)`: float64 brute force after the definition in include/chemeleon_hip.h (chm_dedup_*):
    every lattice translation inside the plane-spacing bound (no cap), the 6 sigma support, the cosine taper.
    The yardstick of the GPU tests.
  * `fingerprint_f32(...)`: the same in float32 numpy in the documented operation order (distance as the
    screen's, t = d - r_k, exp(-(t t) / (2 sigma^2)) taper [z_i z_j], sequential sums). It is the baseline of
    the error gate: the device may miss float64 by 16 x what this restatement misses it by.
  * `distance`, `match_matrix`, `leader`: the match and leader rules in plain Python over a distance matrix.
  * builders: seeded random cells and their copies under permutation, translation, rotation, unimodular basis
    change and supercells (the same crystal), and copies with one atom moved by 0.3 A (another crystal).

Shapes are small because the kernels' risks are boundaries: crystals of 1, 2, 63, 64, 65 (wave), 127, 128, 129
atoms (the staging tile of 128: tile and tile-pair paths), batches of 1, 2, 33, 65, 130 fingerprints (the bit
matrix's words of 32 and the 32 x 32 pair tiles).
"""

import functools
import math

import numpy as np

TOL, R_CUT, SIGMA, BINS = 0.05, 6.0, 0.15, 64
SUPPORT = 6.0   # in sigma
MAX_RANGE = 8   # the kernel's cap of the image range per axis
TILE = 128      # the kernel's staging tile
DEGENERATE, NONFINITE = 8, 16
TI, O, SR = 22, 8, 38


# ------------------------------------------------------------------------------------------ shared pieces
def clamp_types(types):
    t = np.asarray(types, dtype=np.int64)
    return np.where((t >= 0) & (t <= 103), t, 0)


def reduced_counts(types):
    cnt = np.bincount(clamp_types(types), minlength=104).astype(np.int64)
    g = 0
    for c in cnt:
        g = math.gcd(g, int(c))
    return (cnt // g).astype(np.int32)


def image_bounds(lattice, r_cut=R_CUT):
    """(r [3]: the bounds (0.5 + r_cut / h_k)(1 + 1e-5) in float64, volume)."""
    L = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    cr = [np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])]
    vol = abs(float(np.dot(L[0], cr[0])))
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.array([vol / np.linalg.norm(c) for c in cr])
        r = (0.5 + r_cut / h) * (1.0 + 1.0e-5)
    return r, vol


def flags_of(lattice, frac, r_cut=R_CUT):
    """The flags of a crystal by the header's rules (float64)."""
    L, f = np.asarray(lattice, dtype=np.float64), np.asarray(frac, dtype=np.float64)
    fl = 0
    if not (np.all(np.isfinite(L)) and np.all(np.isfinite(f))):
        fl |= NONFINITE
    r, vol = image_bounds(L, r_cut)
    if not vol > 0 or not np.all(r < MAX_RANGE + 1):
        fl |= DEGENERATE
    return fl


def _fingerprint(lattice, frac, types, K, r_cut, sigma, dt):
    """The definition in dtype `dt` -> fp [2K] (zeros for a flagged crystal)."""
    f = dt
    L = np.asarray(lattice).astype(f).reshape(3, 3)
    x = np.asarray(frac).astype(f).reshape(-1, 3)
    z = clamp_types(types)
    n = len(z)
    out = np.zeros(2 * K, dtype=f)
    if flags_of(lattice, frac, r_cut):
        return out
    r, _ = image_bounds(L, r_cut)
    R = [int(math.floor(v)) for v in r]
    w = x[None, :, :] - x[:, None, :]          # [i, j] = x_j - x_i
    w = (w - np.rint(w)).astype(f)
    zz = (z[:, None] * z[None, :]).astype(f)
    self_pair = np.eye(n, dtype=bool)
    rk = ((np.arange(K).astype(f) + f(0.5)) * (f(r_cut) / f(K))).astype(f)
    cut = f(SUPPORT) * f(sigma)
    inv2s2 = f(1.0) / ((f(2.0) * f(sigma)) * f(sigma))
    acc0, acc1 = np.zeros(K, dtype=f), np.zeros(K, dtype=f)
    for n0 in range(-R[0], R[0] + 1):
        for n1 in range(-R[1], R[1] + 1):
            for n2 in range(-R[2], R[2] + 1):
                v = (w + np.array([n0, n1, n2], dtype=f)).astype(f)
                c = ((v[..., 0:1] * L[0] + v[..., 1:2] * L[1]).astype(f) + v[..., 2:3] * L[2]).astype(f)
                d = np.sqrt(((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]).astype(f) + c[..., 2] * c[..., 2]).astype(f))
                hit = d <= f(r_cut)
                if n0 == 0 and n1 == 0 and n2 == 0:
                    hit &= ~self_pair
                if not hit.any():
                    continue
                dh, zh = d[hit].astype(f), zz[hit]
                taper = (f(0.5) * (f(1.0) + np.cos((f(math.pi) * dh) / f(r_cut)).astype(f))).astype(f)
                t = (dh[:, None] - rk[None, :]).astype(f)
                g = (np.exp((-(t * t) * inv2s2).astype(f)).astype(f) * taper[:, None]).astype(f)
                g = np.where(np.abs(t) <= cut, g, f(0.0)).astype(f)
                # (sequential sums over the pairs, as a thread of the kernel adds them)
                acc0 = (acc0 + np.cumsum(g, axis=0, dtype=f)[-1]).astype(f)
                acc1 = (acc1 + np.cumsum((g * zh[:, None]).astype(f), axis=0, dtype=f)[-1]).astype(f)
    zs = f(z.sum())
    out[:K] = acc0 * (f(1.0) / f(n))
    out[K:] = acc1 * (f(n) / (zs * zs)) if z.sum() > 0 else f(0.0)
    return out


def fingerprint_f64(lattice, frac, types, K=BINS, r_cut=R_CUT, sigma=SIGMA):
    return _fingerprint(lattice, frac, types, K, r_cut, sigma, np.float64)


def fingerprint_f32(lattice, frac, types, K=BINS, r_cut=R_CUT, sigma=SIGMA):
    return _fingerprint(np.asarray(lattice, dtype=np.float32), np.asarray(frac, dtype=np.float32), types, K, r_cut,
                        sigma, np.float32)


def rel_error(F, F64):
    return float(np.linalg.norm(np.asarray(F, dtype=np.float64) - F64) / np.linalg.norm(F64))


def distance(Fa, Fb):
    """|F_a - F_b| / max(|F_a|, |F_b|) in float64 (0 for two zero fingerprints)."""
    a, b = np.asarray(Fa, dtype=np.float64), np.asarray(Fb, dtype=np.float64)
    m = max(np.linalg.norm(a), np.linalg.norm(b))
    return 0.0 if m == 0 else float(np.linalg.norm(a - b) / m)


def distance_matrix(F):
    B = len(F)
    D = np.zeros((B, B))
    for g in range(B):
        for h in range(g + 1, B):
            D[g, h] = D[h, g] = distance(F[g], F[h])
    return D


def match_matrix(D, counts, ok, tol=TOL):
    """match[g][h] for g != h: both usable, equal reduced counts, distance <= tol."""
    B = len(D)
    M = np.zeros((B, B), dtype=bool)
    for g in range(B):
        for h in range(B):
            M[g, h] = g != h and ok[g] and ok[h] and np.array_equal(counts[g], counts[h]) and D[g, h] <= tol
    return M


def leader(match, ok=None):
    """The leader rule of group_structures over a match matrix -> (group [B], count [B])."""
    B = len(match)
    ok = [True] * B if ok is None else ok
    group, count, reps = [-1] * B, [0] * B, []
    for g in range(B):
        if not ok[g]:
            continue
        mine = [r for r in reps if match[r][g]]
        if mine:
            group[g] = mine[0]
            count[mine[0]] += 1
        else:
            reps.append(g)
            group[g] = g
            count[g] = 1
    return np.array(group, dtype=np.int32), np.array(count, dtype=np.int32)


# ------------------------------------------------------------------------------------------ builders
def crystal(lattice, frac, types, name=""):
    return dict(name=name, lattice=np.asarray(lattice, dtype=np.float64).reshape(3, 3),
                frac=np.asarray(frac, dtype=np.float64).reshape(-1, 3), types=np.asarray(types, dtype=np.int64).reshape(-1))


def random_cell(rng, n, per_atom=14.0):
    """A triclinic cell of about per_atom A^3 per atom, angles within 75..105 degrees, randomly rotated."""
    s = (n * per_atom) ** (1.0 / 3.0)
    a, b, c = s * rng.uniform(0.85, 1.15, 3)
    al, be, ga = np.radians(rng.uniform(75, 105, 3))
    cx = math.cos(be)
    cy = (math.cos(al) - math.cos(be) * math.cos(ga)) / math.sin(ga)
    L = np.array([[a, 0, 0], [b * math.cos(ga), b * math.sin(ga), 0], [c * cx, c * cy, c * math.sqrt(1 - cx * cx - cy * cy)]])
    return L @ random_rotation(rng)


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def random_crystal(seed, types, name=""):
    rng = np.random.default_rng(seed)
    types = np.asarray(types, dtype=np.int64)
    return crystal(random_cell(rng, len(types)), rng.random((len(types), 3)), types, name or f"random{seed}")


def permuted(c, rng):
    p = rng.permutation(len(c["types"]))
    return crystal(c["lattice"], c["frac"][p], c["types"][p], c["name"] + "+perm")


def translated(c, rng):
    return crystal(c["lattice"], np.mod(c["frac"] + rng.random(3), 1.0), c["types"], c["name"] + "+shift")


def rotated(c, rng):
    return crystal(c["lattice"] @ random_rotation(rng), c["frac"], c["types"], c["name"] + "+rot")


def rebased(c, rng):
    """Another basis of the same lattice: L' = U L with U an integer matrix of determinant +-1 (two shears and
    a permutation of the rows), frac' = frac U^-1."""
    U = np.eye(3)
    for _ in range(2):
        i, j = rng.choice(3, size=2, replace=False)
        S = np.eye(3)
        S[i, j] = rng.choice([-1.0, 1.0])
        U = S @ U
    U = U[rng.permutation(3)]
    assert abs(abs(np.linalg.det(U)) - 1.0) < 1e-12
    return crystal(U @ c["lattice"], np.mod(c["frac"] @ np.linalg.inv(U), 1.0), c["types"], c["name"] + "+basis")


def supercell(c, reps, name=None):
    reps = np.asarray(reps)
    shifts = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), -1).reshape(-1, 3)
    frac = np.concatenate([(c["frac"] + s) / reps for s in shifts])
    return crystal(c["lattice"] * reps[:, None], frac, np.tile(c["types"], len(shifts)),
                   name or c["name"] + "+%dx%dx%d" % tuple(reps))


TRANSFORMS = {"perm": permuted, "shift": translated, "rot": rotated, "basis": rebased,
              "2x1x1": lambda c, rng: supercell(c, (2, 1, 1)), "1x2x2": lambda c, rng: supercell(c, (1, 2, 2))}


def same_crystal(c, seed):
    """c under a random combination of the transformations (at least one), at most one supercell."""
    rng = np.random.default_rng(seed)
    kinds = [k for k in ("perm", "shift", "rot", "basis") if rng.random() < 0.6]
    if rng.random() < 0.5:
        kinds.insert(int(rng.integers(0, len(kinds) + 1)), str(rng.choice(["2x1x1", "1x2x2"])))
    if not kinds:
        kinds = ["perm"]
    for k in kinds:
        c = TRANSFORMS[k](c, rng)
    return c


def perturbed(c, seed, by=0.3):
    """c with one atom moved by `by` A in a random direction: another crystal."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(3)
    v *= by / np.linalg.norm(v)
    frac = c["frac"].copy()
    i = int(rng.integers(len(frac)))
    frac[i] = np.mod(frac[i] + v @ np.linalg.inv(c["lattice"]), 1.0)
    return crystal(c["lattice"], frac, c["types"], c["name"] + "+moved")


def batch_arrays(cs):
    """(natoms, atom_types [N] int64, frac [N,3] f32, lattices [B,3,3] f32) of a list of crystals."""
    return ([len(c["types"]) for c in cs], np.concatenate([c["types"] for c in cs]).astype(np.int64),
            np.concatenate([c["frac"] for c in cs]).astype(np.float32),
            np.stack([c["lattice"] for c in cs]).astype(np.float32))


def reference(cs):
    """Per crystal of the list, from its float32 inputs (what the device sees): float64 fingerprints [B,2K],
    reduced counts [B,104], flags [B]."""
    F, C, fl = [], [], []
    for c in cs:
        L, x = c["lattice"].astype(np.float32), c["frac"].astype(np.float32)
        F.append(fingerprint_f64(L, x, c["types"]))
        C.append(reduced_counts(c["types"]))
        fl.append(flags_of(L, x))
    return np.stack(F), np.stack(C), np.array(fl, dtype=np.int32)


# ------------------------------------------------------------------------------------------ fingerprint cases
@functools.lru_cache(maxsize=None)
def fingerprint_cases():
    """The ragged batch of the fingerprint tests."""
    rng = np.random.default_rng(20261020)
    out = []
    cubic = lambda a: np.eye(3) * a  # noqa: E731
    out.append(crystal(cubic(3.0), [[0.2, 0.4, 0.6]], [TI], "n1_self_images"))
    out.append(crystal(random_cell(rng, 2, 20.0), rng.random((2, 3)), [TI, O], "n2"))
    for n in (63, 64, 65, TILE - 1, TILE, TILE + 1):
        out.append(crystal(random_cell(rng, n), rng.random((n, 3)), rng.choice([TI, O, SR], size=n), f"n{n}"))
    out.append(crystal(cubic(4.0), [[1e-6, 0.3, 0.3], [0.999999, 0.3, 0.3], [0.5, 0.8, 0.1]], [TI, O, O], "wrap"))
    # a pair 5e-5 A inside r_cut (the taper leaves about 2e-10 of it) beside a pair at 1.5 A
    out.append(crystal(cubic(20.0), [[0.1, 0.1, 0.1], [0.1 + (R_CUT - 5e-5) / 20.0, 0.1, 0.1], [0.1, 0.175, 0.1]],
                       [TI, O, O], "taper"))
    thin = lambda a: np.diag([a, 10.0, 10.0])  # noqa: E731
    out.append(crystal(thin(2.0), [[0.1, 0.2, 0.3], [0.6, 0.45, 0.4]], [TI, O], "thin_R3"))
    out.append(crystal(thin(0.75), [[0.1, 0.2, 0.3], [0.6, 0.45, 0.4]], [TI, O], "thin_R8"))
    out.append(crystal(thin(0.6), [[0.1, 0.2, 0.3], [0.6, 0.45, 0.4]], [TI, O], "beyond_cap"))
    out.append(crystal([[4.0, 0, 0], [0, 5.0, 0], [4.0, 5.0, 0]], [[0.1, 0.1, 0.1], [0.4, 0.4, 0.2]], [TI, O],
                       "zero_volume"))
    out.append(crystal(cubic(5.0), [[0.1, 0.1, 0.1], [0.5, float("nan"), 0.5], [0.1, 0.6, 0.6]], [TI, O, O],
                       "nan_coordinate"))
    out.append(crystal(cubic(5.0), [[0.1, 0.1, 0.1], [0.5, 0.5, 0.5], [0.1, 0.6, 0.6], [0.7, 0.2, 0.9]],
                       [TI, O, 104, -3], "class_outside"))
    out.append(crystal(cubic(4.5), rng.random((5, 3)), [0] * 5, "all_class_0"))
    return out


@functools.lru_cache(maxsize=None)
def fingerprint_reference():
    return reference(fingerprint_cases())


@functools.lru_cache(maxsize=None)
def baseline_errors():
    """name -> relative error of the float32 restatement against float64, for the unflagged cases."""
    F64, _, fl = fingerprint_reference()
    return {c["name"]: rel_error(fingerprint_f32(c["lattice"], c["frac"], c["types"]), F64[g])
            for g, c in enumerate(fingerprint_cases()) if fl[g] == 0}


def error_gate():
    """16 x the largest error of the float32 restatement (the ratio step_cases uses against float32 baselines)."""
    return 16.0 * max(baseline_errors().values())


# ------------------------------------------------------------------------------------------ grouping cases
TIO2 = [TI, TI, O, O, O, O]
GROUP_SIZES = (1, 2, 33, 65, 130)


def _f64(c):
    return fingerprint_f64(c["lattice"], c["frac"], c["types"])


def distinct_from(make, seed, others):
    """make(seed'), for the first seed' = seed, seed + 7919, ... whose crystal is further than 2.2 tol from every
    fingerprint in `others` (the margin condition of the grouping tests is a condition on the inputs: the seeds
    are chosen to meet it) -> (crystal, its float64 fingerprint)."""
    for q in range(400):
        c = make(seed + 7919 * q)
        F = _f64(c)
        if all(distance(F, G) > 2.2 * TOL for G in others):
            return c, F
    raise AssertionError("no seed keeps the crystal clear of the others")


@functools.lru_cache(maxsize=None)
def planted(B, seed=7):
    """B crystals with planted membership: originals (Ti2O4 cells, and every fourth a SrTiO3 cell) each followed
    by 0-4 relatives (the same crystal transformed, or with one atom moved 0.3 A), then interleaved by a seeded
    shuffle -> (crystals, labels): equal labels = the same crystal. Different crystals of one composition are
    further than 2.2 tol apart (distinct_from)."""
    rng = np.random.default_rng(1000 * B + seed)
    cs, labels, k = [], [], 0
    known = {}  # composition -> fingerprints of the different crystals so far
    while len(cs) < B:
        types = [SR, TI, O, O, O] if k % 4 == 3 else TIO2
        fam = known.setdefault(len(types), [])
        orig, F = distinct_from(lambda sd: random_crystal(sd, types, f"orig{k}"), int(rng.integers(1 << 30)), fam)
        fam.append(F)
        cs.append(orig)
        labels.append(k)
        for _ in range(int(rng.integers(0, 5))):
            if len(cs) >= B:
                break
            if rng.random() < 0.75:
                cs.append(same_crystal(orig, int(rng.integers(1 << 30))))
                labels.append(k)
            else:
                moved, F = distinct_from(lambda sd: perturbed(orig, sd), int(rng.integers(1 << 30)), fam)
                fam.append(F)
                cs.append(moved)
                labels.append(-len(cs))  # a crystal of its own
        k += 1
    order = rng.permutation(B)
    return [cs[i] for i in order], [labels[i] for i in order]


@functools.lru_cache(maxsize=None)
def planted_reference(B):
    """(F64 [B,2K], counts, flags, D [B,B], group, count) of planted(B) by the plain rules."""
    cs, _ = planted(B)
    F, C, fl = reference(cs)
    D = distance_matrix(F)
    ok = fl == 0
    group, count = leader(match_matrix(D, C, ok), ok)
    return F, C, fl, D, group, count


@functools.lru_cache(maxsize=None)
def invariance_cases():
    """[(original, [same crystals], [moved copies])]: every transformation alone, then random combinations; the
    moved copies (one atom by 0.3 A) are further than 2.2 tol from the original and from each other."""
    out = []
    for k, types in enumerate([TIO2, [SR, TI, O, O, O], [TI, TI, TI, O, O, O, O, O]]):
        orig = random_crystal(300 + k, types, f"inv{k}")
        rng = np.random.default_rng(400 + k)
        same = [TRANSFORMS[name](orig, rng) for name in TRANSFORMS] + [same_crystal(orig, 500 + 10 * k + q) for q in range(3)]
        fam, moved = [_f64(orig)], []
        for q in range(2):
            m, F = distinct_from(lambda sd: perturbed(orig, sd), 600 + 10 * k + q, fam)
            fam.append(F)
            moved.append(m)
        out.append((orig, same, moved))
    return out


def swapped_elements():
    """Two crystals of equal geometry and composition TiO with the two elements exchanged, and a third of equal
    geometry and another composition (Ti2): only the types differ."""
    rng = np.random.default_rng(77)
    L, x = random_cell(rng, 4), rng.random((4, 3))
    return [crystal(L, x, [TI, TI, O, O], "TiTiOO"), crystal(L, x, [O, O, TI, TI], "OOTiTi"),
            crystal(L, x, [TI, TI, TI, TI], "Ti4")]
