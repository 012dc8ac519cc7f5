"""Shared inputs of the tests of grouping by matching (chemeleon_amd.match_group, csrc/match.hip: chm_match_group_*).

Expected results come from the restatement of tests/match_cases.py (imported, not edited): `pair(h, g, dtype)` is
restate(sample = crystal g, ref = crystal h) of two named crystals, computed once per ordered pair and shared; the
match matrix of a batch is that over every h < g of equal atom count, and `expected(batch)` applies the plain leader
rule to it in Python: in index order a crystal joins the earliest earlier representative it matches, else it is one.

The crystals (POOL, 65 of them, interleaved so that the representatives are spread over the batch): for each of
match_cases' references but simple cubic (CsCl, rock salt in both cells, diamond, rutile, wurtzite, alpha-quartz, the
P1 cell) the structure itself, a disguised copy (a seeded rotation, unimodular basis change, permutation and origin
shift at once), displacements of 0.05 A, a copy scaled 0.9 or 1.1, a 5% strain, and the non-duplicates: one atom
moved by 1.0 A and the 0.7 compression; quartz's mirror image; rutile with one Ti and one O exchanged; two simple-
cubic cells (the only pair at n = 1), the 65-atom supercell and its displaced copy (the only pair at n = 65), a
3-atom P1 cell (a size that occurs once), a zero-volume lattice (group -1), and two copies of a thin 7-atom cell
(the pair sets THIN: neither joins the other).

The batches (batches()): the first 1, 31, 32, 33 and 65 crystals of POOL (the bit matrix's word edges), two rutile
copies (B = 2), the first 33 with an exclusion mask that takes out a representative and a member, and the
non-transitive chain in both orders: A, B = A + v, C = A + 2 v with A ~ B, B ~ C but not A ~ C, so A, B, C gives
{A, B}, {C} and B, A, C gives {B, A, C}.
"""

import functools

import numpy as np

from tests import cell_cases as cc
from tests import match_cases as M
from tests import symmetry_cases as sc

EXCLUDED = 64
STRUCTURES = M.REFERENCES[1:]
# the chain: per-atom displacements of CHAIN_AMPLITUDE A in seeded directions, applied once (B) and twice (C)
CHAIN_BASE, CHAIN_SEED, CHAIN_AMPLITUDE = "p1_five", 7, 0.45


def _moved(struct, v):
    L, types, frac = struct
    return L, types, np.mod(frac + v @ np.linalg.inv(L), 1.0)


@functools.lru_cache(maxsize=None)
def _build():
    """(crystals: name -> structure dict, POOL: the names in batch order)."""
    base = sc._base_structures()
    tri = cc.cell(4.0, 5.3, 6.7, 78, 97, 109)
    base["p1_five"] = (tri, np.array([20, 8, 8, 6, 6]), np.array([[.05, .11, .23], [.31, .62, .17], [.55, .29, .71],
                                                                   [.83, .47, .39], [.19, .88, .64]]))
    rng = np.random.default_rng(20261021)
    raw, per = {}, []
    for s, name in enumerate(STRUCTURES):
        L, types, frac = base[name]
        raw[name] = base[name]
        raw[f"{name}_variant"] = sc._variant(base[name], rng)
        raw[f"{name}_d005"] = M.displaced(base[name], 0.05, 300 + s)[0]
        raw[f"{name}_strain30"] = (L @ np.diag([0.7, 1, 1]), types, frac)
        u = rng.standard_normal(3)
        x = np.array(frac, dtype=np.float64)
        x[-1] = x[-1] + (u / np.linalg.norm(u)) @ np.linalg.inv(L)
        raw[f"{name}_moved1"] = (L, types, x)
        scaled = "scale09" if s % 2 == 0 else "scale11"
        raw[f"{name}_{scaled}"] = sc._variant(((0.9 if s % 2 == 0 else 1.1) * L, types, frac), rng)
        kinds = ["", "_variant", "_d005", "_strain30", "_moved1", "_" + scaled]
        if s < len(STRUCTURES) - 1:
            raw[f"{name}_strain5"] = sc._variant((L @ np.diag([1.05, 1, 1]), types, frac), rng)
            kinds.append("_strain5")
        per.append([name + kinds[(k + s) % len(kinds)] for k in range(len(kinds))])
    L, types, frac = base["quartz"]
    raw["quartz_mirror"] = (L @ cc.rotation(rng), types, np.mod(-frac, 1.0))
    L, types, frac = base["rutile"]
    swapped = types.copy()
    ti, ox = int(np.flatnonzero(types == 22)[0]), int(np.flatnonzero(types == 8)[0])
    swapped[ti], swapped[ox] = 8, 22
    raw["rutile_exchanged"] = (L, swapped, frac)
    raw["sc1"] = base["simple_cubic"]
    raw["sc1_scale11"] = sc._variant((1.1 * base["simple_cubic"][0],) + tuple(base["simple_cubic"][1:]), rng)
    L, types, frac = sc._supercell_sc(3.0, (4, 4, 4))
    raw["sc_65"] = (L, np.append(types, 8), np.vstack([frac, [[.125, .125, .125]]]))
    raw["sc_65_d005"] = M.displaced(raw["sc_65"], 0.05, 204)[0]
    raw["p1_three"] = base["p1"]
    raw["zero_volume"] = ([[4.1, 0, 0], [0, 4.1, 0], [4.1, 4.1, 0]],) + tuple(base["cscl"][1:])
    thin = (cc.cell(4, 5.2, 0.19, 90, 90, 90), np.array([29, 29, 29, 8, 8, 8, 8]),
            np.array([[.1, .1, 0], [.6, .2, .3], [.3, .7, .6], [.8, .8, .1], [.45, .4, .8], [.05, .55, .5], [.7, .5, .9]]))
    raw["thin_a"] = thin
    raw["thin_b"] = (thin[0], thin[1], np.mod(thin[2] + [.21, .13, .4], 1.0))
    # the chain
    rs = np.random.default_rng(CHAIN_SEED)
    v = rs.standard_normal(np.shape(base[CHAIN_BASE][2]))
    v *= CHAIN_AMPLITUDE / np.linalg.norm(v, axis=1, keepdims=True)
    raw["chain_a"] = base[CHAIN_BASE]
    raw["chain_b"] = _moved(base[CHAIN_BASE], v)
    raw["chain_c"] = _moved(base[CHAIN_BASE], 2 * v)
    # interleave: round k takes the k-th entry of every structure's list, the extras at fixed places
    order = [per[s][k] for k in range(max(len(p) for p in per)) for s in range(len(per)) if k < len(per[s])]
    for at, name in ((2, "sc1"), (5, "zero_volume"), (11, "thin_a"), (14, "p1_three"), (20, "thin_b"), (26, "sc_65"),
                     (29, "sc1_scale11"), (36, "quartz_mirror"), (40, "sc_65_d005"), (44, "rutile_exchanged")):
        order.insert(at, name)
    assert len(order) == 65 and len(set(order)) == 65, len(order)
    return {name: M._structure(*s) for name, s in raw.items()}, tuple(order)


def crystals():
    return _build()[0]


def pool():
    return _build()[1]


def usable(name) -> bool:
    """Has the crystal a reduced cell? (else it gets group -1 and none of its pairs is searched)"""
    return M.reduced(crystals()[name]["lattice"]) is not None


@functools.lru_cache(maxsize=None)
def pair(h, g, dtype_name="float64"):
    """The restatement's record of crystal g (the sample) against crystal h (the reference). Shared: do not modify."""
    dt = np.float32 if dtype_name == "float32" else np.float64
    return M.restate(crystals()[g], crystals()[h], dt)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (crystal names in batch order, exclusion mask as a bool array or None)."""
    p = pool()
    mask = np.zeros(33, dtype=bool)
    mask[[0, 9, 17]] = True
    out = {f"first{B}": (p[:B], None) for B in (1, 31, 32, 33, 65)}
    out["two"] = (("rutile_d005", "rutile_variant"), None)
    out["excluded"] = (p[:33], mask)
    out["chain_abc"] = (("chain_a", "chain_b", "chain_c"), None)
    out["chain_bac"] = (("chain_b", "chain_a", "chain_c"), None)
    return out


def pairs_of(names):
    """[(h, g)] positions: every h < g of equal atom count, ordered by g, then h (the plan's pair order)."""
    n = [len(crystals()[c]["types"]) for c in names]
    return [(h, g) for g in range(len(names)) for h in range(g) if n[h] == n[g]]


@functools.lru_cache(maxsize=None)
def expected(batch, dtype_name="float64"):
    """dict(pairs [(h, g)], records: per pair the restatement's record or None where the pair is not searched (an
    excluded crystal or one without a reduced cell), matched [P] bool, group [B], count [B])."""
    names, mask = batches()[batch]
    B = len(names)
    out_of = [bool(mask is not None and mask[g]) or not usable(names[g]) for g in range(B)]
    prs = pairs_of(names)
    records = [None if out_of[h] or out_of[g] else pair(names[h], names[g], dtype_name) for h, g in prs]
    matched = np.array([r is not None and bool(r["matched"]) for r in records], dtype=bool)
    hit = {pr for pr, m in zip(prs, matched) if m}
    group, count, reps = np.full(B, -1, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for g in range(B):
        if out_of[g]:
            continue
        lead = next((r for r in reps if (r, g) in hit), g)
        if lead == g:
            reps.append(g)
        group[g] = lead
        count[lead] += 1
    return dict(pairs=prs, records=records, matched=matched, group=group, count=count)


def float32_error():
    """The largest |float32 - float64| of rms and max_dist over every searched pair of every batch."""
    worst = 0.0
    for b in batches():
        for a, c in zip(expected(b, "float32")["records"], expected(b, "float64")["records"]):
            if a is not None:
                worst = max(worst, abs(a["rms"] - c["rms"]), abs(a["max_dist"] - c["max_dist"]))
    return worst


def packed(batch):
    """(natoms, types int64 [N], frac float32 [N,3], lattices float32 [B,3,3], mask or None) of a batch."""
    names, mask = batches()[batch]
    return M.packed([crystals()[c] for c in names]) + (mask,)
