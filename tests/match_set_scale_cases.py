"""Shared inputs of the tests of the reference-set search at the scale where a block of k_set_pairs (csrc/match.hip)
runs several pairs and k_set_offsets scans more than one round: 300 samples against 99 references, built on the
restatements of tests/match_cases.py (nearest partners) and tests/assign_cases.py (assignment) and on the set
definition of tests/match_set_cases.py (key, sort, candidates, winner), all imported and not edited.

The set (reference_names(), 99 structures in a seeded shuffle): 11 buckets of one (atom count, composition) with 9
references each. Eight buckets are seeded low-symmetry cells of 2, 2, 2, 4, 4, 4, 8 and 8 atoms (two lattice
mappings per pair, so a pair costs milliseconds to restate); three are the collision structures "three" (3 atoms),
"blocks_of_one" (4) and "chain" (5) of tests/assign_cases.py, whose nearest partners collide. A bucket holds its
parent, the parent displaced by 0.03 A, scaled 1.08 and displaced by 0.05 A, strained 4% and displaced by 0.02 A,
compressed to 0.7 along a, with one atom moved by 1.0 A, with two atoms of different species exchanged (or, with a
single species pair, a second atom moved), on a zero-volume lattice (no reduced cell) and on a thin cell (THIN): the
last two are the early exits of every sample of the bucket.

The samples (batch(), B = 300 in a seeded shuffle): per bucket disguised copies (a seeded rotation, unimodular basis
change, permutation and origin shift at once) of the parent and of its scaled reference displaced by 0.03 to 0.06 A
(they match several references), of the compressed, the moved and the exchanged reference (they match that one), of
the parent strained 30% along b or with another atom moved by 1.0 A (they match none); in the collision buckets most
samples are disguised copies of the collision sample displaced by up to 0.02 A (collided candidates: the assignment
pairing solves them, the nearest rule drops them). 64 samples have no candidate: compositions the set does not hold
(sizes it holds), sizes it does not hold (1, 6 and 7 atoms) and zero-volume lattices; twelve of them are put at
indices 250 to 261, across the scan's round boundary, and the exclusion mask MASKED takes samples on both sides of
it. A sample is drawn again (the next seed) until, against every one of its candidates and in both pairings, every
deciding quantity stays MARGIN of its bound away in float64, float32 and float64 agree on matched, flags and the
counts, and its best and second-best matched rms differ by GAP (ten times the GPU gate): so the cases cannot sit on
a tolerance edge.

Every pair of the batch is restated, in float64 and float32 and in both pairings (2 061 pairs; none is left to the
chunked device runs alone). On one CPU core the float64 restatements of both pairings take 25 s and the float32 ones
34 s, measured and printed by tests/test_match_set_scale_cases.py. The float32 restatement's largest difference from
float64 in rms / max_dist over these pairs is 6.9e-7 under either pairing: the GPU gate is 16 times that, 1.1e-5.

A pair's kind, for the sequences a block sees: EARLY (the restatement returns flags before the search: NO_LATTICE or
THIN), COLLIDED (the assignment restatement solved at least one collided candidate), else MATCHED or UNMATCHED (no
collision: both pairings give the same record).
"""

import functools
import time

import numpy as np

from tests import assign_cases as A
from tests import cell_cases as cc
from tests import match_cases as M
from tests import match_set_cases as S
from tests import symmetry_cases as sc

B = 300
GRID = 768            # 3 blocks x 256 compute units: the pair kernel's grid on an MI355X
P_FLOOR = 2 * GRID + 200
MARGIN = M.MARGIN
GAP = 1.0e-4
MASKED = (5, 77, 140, 201, 249, 252, 258, 263, 290)
PAIRINGS = ("nearest", "assignment")
EARLY, COLLIDED, MATCHED, UNMATCHED = "early", "collided", "matched", "unmatched"
KINDS = (EARLY, COLLIDED, MATCHED, UNMATCHED)
TRANSITIONS = ((COLLIDED, MATCHED), (MATCHED, EARLY), (EARLY, MATCHED), (MATCHED, UNMATCHED))
NEAR_MARGINS = ("lattice_margin", "pair_margin", "gap_margin", "thin_margin")
ASSIGN_MARGINS = NEAR_MARGINS + ("rms_margin",)

# the seeded buckets: (name, cell, types, fractional coordinates)
GENERIC = (
    ("g2a", (3.6, 4.9, 6.7, 80, 97, 108), (11, 17), ((.05, .11, .23), (.47, .58, .66))),
    ("g2b", (3.4, 4.7, 6.4, 83, 101, 111), (12, 8), ((.12, .07, .31), (.61, .49, .83))),
    ("g2c", (3.8, 5.1, 6.9, 79, 99, 106), (30, 16), ((.21, .33, .09), (.68, .81, .57))),
    ("g4a", (4.2, 5.7, 7.7, 81, 98, 109), (22, 8, 8, 8), ((.05, .11, .23), (.31, .62, .17), (.55, .29, .71), (.83, .87, .49))),
    ("g4b", (4.4, 5.9, 8.1, 82, 100, 107), (11, 11, 17, 17), ((.09, .14, .2), (.58, .63, .7), (.33, .78, .41), (.84, .27, .93))),
    ("g4c", (4.0, 5.5, 7.4, 78, 96, 110), (20, 6, 8, 8), ((.15, .05, .3), (.4, .55, .12), (.66, .3, .64), (.9, .8, .85))),
    ("g8a", (5.3, 7.1, 9.7, 80, 99, 108), (13, 13, 15, 15, 15, 15, 8, 8),
     ((.05, .1, .2), (.55, .6, .7), (.3, .15, .55), (.8, .35, .1), (.15, .65, .4), (.65, .85, .9), (.4, .45, .85), (.9, .9, .45))),
    ("g8b", (5.5, 7.5, 10.1, 83, 97, 111), (14, 14, 14, 8, 8, 8, 8, 8),
     ((.1, .05, .15), (.6, .5, .65), (.35, .8, .4), (.2, .3, .75), (.75, .2, .3), (.5, .25, .95), (.85, .7, .1), (.05, .6, .55))),
)
COLLISIONS = ("three", "blocks_of_one", "chain")
N_GENERIC, N_COLLISION = 16, 36  # samples per bucket


# ------------------------------------------------------------------------------------------ the structures
def _moved(struct, atom, seed, dist=1.0):
    L, types, frac = struct
    u = np.random.default_rng(seed).standard_normal(3)
    x = np.array(frac, dtype=np.float64)
    x[atom] = x[atom] + (dist * u / np.linalg.norm(u)) @ np.linalg.inv(L)
    return L, types, np.mod(x, 1.0)


def _exchanged(struct, seed):
    """Two atoms of different species exchanged; with one pair of species in a two-atom cell (where that is an
    inversion) the second atom moved by 0.8 A instead."""
    L, types, frac = struct
    if len(types) == 2:
        return _moved(struct, 1, seed, 0.8)
    t = np.array(types)
    i = int(np.flatnonzero(t != t[0])[0])
    t[0], t[i] = t[i], t[0]
    return L, t, frac


def _references(parent, n, seed):
    """The nine references of a bucket as raw structures, by role."""
    L, types, frac = parent
    d = lambda s, amp, k: M.displaced(s, amp, seed + k)[0]
    return dict(parent=parent, d003=d(parent, 0.03, 1), scaled=d((1.08 * L, types, frac), 0.05, 2),
                strain4=d((L @ np.diag([1.04, 1, 1]), types, frac), 0.02, 3), strain30=(L @ np.diag([0.7, 1, 1]), types, frac),
                moved=_moved(parent, n - 1, seed + 4), exchanged=_exchanged(parent, seed + 5),
                flat=(np.array([[4.1, 0, 0], [0, 4.6, 0], [4.1, 4.6, 0]]), types, frac),
                thin=(cc.cell(4.0, 5.2, 0.3, 90, 90, 90), types, frac))


def _sample_recipes(collision):
    """(role of the source, displacement in A) per sample of a bucket; "none_*" are made from the parent."""
    if collision:
        return ([("collide", a) for a in np.linspace(0.002, 0.02, 24)] + [("parent", 0.03), ("parent", 0.05), ("scaled", 0.03),
                ("d003", 0.02), ("strain30", 0.03), ("moved", 0.03), ("moved", 0.04), ("exchanged", 0.03), ("none_strain", 0.03),
                ("none_moved", 0.03), ("none_moved", 0.05), ("none_strain", 0.0)])
    return [("parent", 0.0), ("parent", 0.03), ("parent", 0.045), ("parent", 0.06), ("scaled", 0.0), ("scaled", 0.04),
            ("strain30", 0.03), ("strain30", 0.05), ("moved", 0.03), ("moved", 0.0), ("exchanged", 0.03), ("exchanged", 0.05),
            ("none_strain", 0.03), ("none_moved", 0.03), ("none_moved", 0.05), ("none_strain", 0.0)]


@functools.lru_cache(maxsize=None)
def pair(sample, ref):
    """The four restatements of `sample` against `ref` (names): {(pairing, dtype name): record}. Shared: do not
    modify. (restate_assign's float64 record carries the nearest rule's float64 record of the same pair.)"""
    st = _structures
    t0 = time.perf_counter()
    a64 = A.restate_assign(st[sample], st[ref], np.float64)
    t1 = time.perf_counter()
    a32 = A.restate_assign(st[sample], st[ref], np.float32)
    n32 = M.restate(st[sample], st[ref], np.float32)
    SECONDS["float64"] += t1 - t0
    SECONDS["float32"] += time.perf_counter() - t1
    return {("assignment", "float64"): a64, ("assignment", "float32"): a32, ("nearest", "float64"): a64["nearest"],
            ("nearest", "float32"): n32}


def _winner_gap(records):
    hits = sorted(r["rms"] for r in records if r["matched"])
    return hits[1] - hits[0] if len(hits) >= 2 else np.inf


def clear_of_every_edge(sample, refs):
    """Does `sample` stay MARGIN from every bound and GAP from a tie against all of `refs`, in both pairings, and do
    float32 and float64 agree on every integer field?"""
    for pairing, fields, margins in (("nearest", M.INT_FIELDS, NEAR_MARGINS), ("assignment", A.INT_FIELDS, ASSIGN_MARGINS)):
        recs = [pair(sample, r) for r in refs]
        for rec in recs:
            r64, r32 = rec[(pairing, "float64")], rec[(pairing, "float32")]
            if any(r64[f] != r32[f] for f in fields) or r64["flags"] & (M.MANY_MAPPINGS | A.MANY_ASSIGNMENTS):
                return False
            if any(r64[m] < MARGIN for m in margins):
                return False
            if any(abs(c[2] - M.STOL) < MARGIN * M.STOL for c in r64["counting"]):
                return False
        for dt in ("float64", "float32"):
            if _winner_gap([rec[(pairing, dt)] for rec in recs]) < GAP:
                return False
    return True


_structures = {}
SECONDS = {"float64": 0.0, "float32": 0.0, "build": 0.0}  # what the restatements took, for the docstring


@functools.lru_cache(maxsize=None)
def _build():
    """(the set's names in original order, the samples' names in batch order, bucket name -> its references' names);
    fills _structures and every pair() of the batch."""
    t0 = time.perf_counter()
    st = _structures
    asg = {c["name"]: c for c in A.cases()}
    buckets, in_set, with_cands, drawn = {}, [], [], 0
    rng = np.random.default_rng(20261101)
    for k, name in enumerate(tuple(g[0] for g in GENERIC) + COLLISIONS):
        collision = name in COLLISIONS
        if collision:
            parent, collide = S._raw(asg[name]["ref"]), S._raw(asg[name]["sample"])
        else:
            _, cell, types, frac = GENERIC[k]
            parent, collide = (cc.cell(*cell), np.array(types), np.array(frac, dtype=np.float64)), None
        n = len(parent[1])
        roles = _references(parent, n, 1000 * (k + 1))
        for role, raw in roles.items():
            st[f"{name}_{role}"] = M._structure(*raw)
        buckets[name] = tuple(f"{name}_{role}" for role in roles)
        in_set += buckets[name]
        sources = dict(roles, collide=collide, none_strain=(parent[0] @ np.diag([1, 0.7, 1]), parent[1], parent[2]),
                       none_moved=_moved(parent, 0, 1000 * (k + 1) + 6))
        recipes = _sample_recipes(collision)
        assert len(recipes) == (N_COLLISION if collision else N_GENERIC)
        for j, (role, amp) in enumerate(recipes):
            for attempt in range(20):  # the next seed until the sample is clear of every edge
                drawn += 1
                raw = sources[role]
                if role == "none_strain":  # (a lattice on an edge stays there whatever the atoms do: another strain)
                    raw = (parent[0] @ np.diag([1, 0.7 - 0.013 * attempt, 1]), parent[1], parent[2])
                if amp:
                    raw = M.displaced(raw, float(amp), 100000 * (k + 1) + 100 * j + attempt)[0]
                s = f"{name}_s{j}" + (f"_draw{attempt}" if attempt else "")
                st[s] = M._structure(*sc._variant(raw, rng))
                if clear_of_every_edge(s, buckets[name]):
                    break
            else:
                raise AssertionError(f"no clear sample for {name} {role} {amp}")
            with_cands.append(s)
    # the samples without a candidate
    assert sorted({len(st[r]["types"]) for r in in_set}) == [2, 3, 4, 5, 8]
    other, size, flat = [], [], []
    for j in range(28):  # compositions the set does not hold, at sizes it holds
        src = st[with_cands[(7 * j) % len(with_cands)]]
        st[f"other{j}"] = M._structure(src["lattice"], src["types"] + 40, src["frac"])
        other.append(f"other{j}")
    for j in range(24):  # sizes the set does not hold
        st[f"size{j}"] = M._structure(*S._filler(rng, (1, 6, 7)[j % 3], np.array([11, 17, 8, 22])))
        size.append(f"size{j}")
    for j in range(12):  # no reduced cell: not searched
        src = st[with_cands[(11 * j + 3) % len(with_cands)]]
        st[f"flat{j}"] = M._structure([[4.1, 0, 0], [0, 4.1, 0], [4.1, 4.1, 0]], src["types"], src["frac"])
        flat.append(f"flat{j}")
    straddle = [v for trio in zip(other[:4], size[:4], flat[:4]) for v in trio]  # a run across the scan's round boundary
    rest = with_cands + other[4:] + size[4:] + flat[4:]
    rest = [rest[k] for k in np.random.default_rng(9).permutation(len(rest))]
    samples = rest[:250] + straddle + rest[250:]
    assert len(samples) == B and len(set(samples)) == B and len(set(in_set)) == len(in_set) == 99
    in_set = [in_set[k] for k in np.random.default_rng(10).permutation(len(in_set))]
    SECONDS["build"] = time.perf_counter() - t0
    return tuple(in_set), tuple(samples), buckets, drawn


def structures():
    _build()
    return _structures


def reference_names():
    return _build()[0]


def batch():
    """(sample names in batch order, the exclusion mask as a bool array)."""
    mask = np.zeros(B, dtype=bool)
    mask[list(MASKED)] = True
    return _build()[1], mask


def usable(name) -> bool:
    return M.reduced(structures()[name]["lattice"]) is not None


@functools.lru_cache(maxsize=None)
def expected(pairing="nearest", dtype_name="float64", masked=True):
    """Per sample of the batch a dict as tests/match_set_cases.expected (key, lo, cands, records, n_candidates,
    n_matched, known, ref, rms, max_dist, flags), under one pairing and dtype. Shared: do not modify."""
    names, st = reference_names(), structures()
    structs = [st[r] for r in names]
    order, _ = S.sort_set(structs)
    samples, mask = batch()
    out = []
    for g, s in enumerate(samples):
        gone, flat = bool(masked and mask[g]), not usable(s)
        rec = dict(key=S.key_of(st[s]["types"]), lo=0, cands=[], records=[], n_candidates=0, n_matched=0, known=False,
                   ref=-1, rms=0.0, max_dist=0.0, flags=(S.EXCLUDED if gone else 0) | (M.NO_LATTICE if flat else 0))
        if not gone and not flat:
            at = S.candidates_of(st[s], structs, order)
            rec["lo"] = at[0] if at else 0
            rec["cands"] = [order[p] for p in at]
            rec["records"] = [pair(s, names[r])[(pairing, dtype_name)] for r in rec["cands"]]
            rec["n_candidates"] = len(at)
            hits = sorted((r["rms"], o) for r, o in zip(rec["records"], rec["cands"]) if r["matched"])
            rec["n_matched"] = len(hits)
            if hits:
                win = rec["records"][rec["cands"].index(hits[0][1])]
                rec.update(known=True, ref=hits[0][1], rms=win["rms"], max_dist=win["max_dist"], flags=win["flags"])
        out.append(rec)
    return out


def kind_of(near, assign):
    """The kind of a pair from its float64 records under the two pairings."""
    if assign["flags"] & ~(M.MANY_MAPPINGS | A.MANY_ASSIGNMENTS):
        return EARLY
    if assign["n_assigned"] > 0:
        return COLLIDED
    assert (near["matched"], near["rms"], near["max_dist"]) == (assign["matched"], assign["rms"], assign["max_dist"])
    return MATCHED if assign["matched"] else UNMATCHED


@functools.lru_cache(maxsize=None)
def kinds():
    """The kind of every pair of the (masked) batch in list order, a tuple of P strings."""
    return tuple(kind_of(n, a) for sn, sa in zip(expected("nearest"), expected("assignment"))
                 for n, a in zip(sn["records"], sa["records"]))


def transitions(grid):
    """{(kind, next kind): blocks that see it}: block b of `grid` runs pairs b, b + grid, b + 2 grid, ..."""
    k = kinds()
    out = {t: 0 for t in TRANSITIONS}
    for b in range(min(grid, len(k))):
        seen = {(k[p], k[p + grid]) for p in range(b, len(k) - grid, grid)}
        for t in TRANSITIONS:
            out[t] += t in seen
    return out


def float32_error(pairing):
    """The largest |float32 - float64| of rms and max_dist over every pair of the batch under `pairing`."""
    worst = 0.0
    for a, c in zip(expected(pairing, "float32"), expected(pairing, "float64")):
        for ra, rc in zip(a["records"], c["records"]):
            worst = max(worst, abs(ra["rms"] - rc["rms"]), abs(ra["max_dist"] - rc["max_dist"]))
    return worst


def gate():
    """The GPU gate: 16 times the float32 restatement's own largest error, over both pairings."""
    return 16 * max(float32_error(p) for p in PAIRINGS)


def packed_set():
    return M.packed([structures()[r] for r in reference_names()])


def packed(names):
    return M.packed([structures()[c] for c in names])


def scan_batch(n):
    """The batch truncated or extended by repeating its samples to n names."""
    names = batch()[0]
    return tuple(names[k % B] for k in range(n))


def size_preserving_permutation(seed):
    """A seeded permutation of range(B) that keeps every position's atom count."""
    names, st = batch()[0], structures()
    sizes = np.array([len(st[s]["types"]) for s in names])
    perm = np.arange(B)
    rng = np.random.default_rng(seed)
    for n in np.unique(sizes):
        at = np.flatnonzero(sizes == n)
        perm[at] = rng.permutation(at)
    return perm
