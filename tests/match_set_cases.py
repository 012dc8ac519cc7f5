"""Shared inputs of the tests of the reference-set search (chemeleon_amd.match_set, csrc/match.hip: chm_match_set_*)
and its definition (include/chemeleon_hip.h) restated in numpy: the composition key, the sort of the set by (atom
count, key, original index), the candidates of a sample as the range of equal (atom count, key), and per candidate
the restatement of tests/match_cases.py (imported, not edited): `pair(sample, ref, dtype)` is restate(sample, ref) of
two named structures, computed once per pair and shared. The winner is the matched candidate with the smallest rms,
ties to the smallest original index.

The set (reference_names(), 70 structures in a seeded shuffle, so that sorted and original order differ): the
references of match_cases (sizes 1, 2, 4, 5, 6, 8, 9, 63, 64, 65 and 256; n = 63, 64, 65 and 256 occur once), for
each of its structures but simple cubic also match_group_cases' copy displaced by 0.05 A and its 0.7 compression, a
second, byte-identical rutile (the exact tie: whichever of the two has the smaller original index wins), quartz
displaced by 0.02 A (a disguised copy of it must take it, not quartz, and the other way round), CsCl on a
zero-volume lattice (a candidate of every CsCl sample that matches nothing) and 35 seeded triclinic fillers of 4, 6,
7, 8, 9 and 11 atoms whose compositions occur nowhere else.

The samples (pool(), 65 of them in a seeded shuffle; batches() takes the first 1, 2, 33 and 65, and 33 with an
exclusion mask): of every structure a disguised copy (a seeded rotation, unimodular basis change, permutation and
origin shift at once), a disguised copy scaled 0.9 or 1.1, a second disguise, a copy displaced by 0.05 A with another
seed (but for quartz), the 5% strain and one atom moved by 1.0 A (match_group_cases' crystals); the disguised displaced quartz;
quartz's mirror image; rutile with one Ti and one O exchanged (the same composition: a candidate that is rejected);
the thin cell (its pair sets THIN); the supercells of 63, 64, 65 and 256 atoms displaced; a 3-atom cell (a size the
set does not hold); CsCl with both atoms Cs and four fillers' cells with other elements (sizes the set holds,
compositions it does not); and a zero-volume lattice (no reduced cell: not searched).
"""

import functools

import numpy as np

from tests import cell_cases as cc
from tests import match_cases as M
from tests import match_group_cases as G
from tests import symmetry_cases as sc

EXCLUDED = 64
MIX_A, MIX_B = np.uint64(0xbf58476d1ce4e5b9), np.uint64(0x94d049bb133111eb)
GAP = 1.0e-3  # between the best and the second-best matched rms of a sample
TWINS = ("rutile", "rutile_twin")


# ------------------------------------------------------------------------------------------ the definition
def mix(types):
    """The splitmix64 finaliser of t + 1, t the type's low 32 bits: uint64, elementwise."""
    with np.errstate(over="ignore"):
        z = (np.asarray(types).astype(np.int64) & 0xffffffff).astype(np.uint64) + np.uint64(1)
        z = (z ^ (z >> np.uint64(30))) * MIX_A
        z = (z ^ (z >> np.uint64(27))) * MIX_B
        return z ^ (z >> np.uint64(31))


def key_of(types) -> int:
    """The composition key as a Python int: the sum of mix over the atoms modulo 2^64."""
    return sum(int(v) for v in mix(types)) % (1 << 64)


def sort_set(structs):
    """(order, keys): the original indices of `structs` sorted ascending by (atom count, key, original index), and
    the keys in that order."""
    rows = sorted((len(s["types"]), key_of(s["types"]), k) for k, s in enumerate(structs))
    return [r[2] for r in rows], [r[1] for r in rows]


def candidates_of(sample, structs, order):
    """The sorted positions of the references with the sample's atom count and key: one contiguous range."""
    n, key = len(sample["types"]), key_of(sample["types"])
    at = [p for p, r in enumerate(order) if len(structs[r]["types"]) == n and key_of(structs[r]["types"]) == key]
    assert at == list(range(at[0], at[0] + len(at))) if at else True
    return at


# ------------------------------------------------------------------------------------------ the structures
def _raw(s):
    return s["lattice"].astype(np.float64), s["types"], s["frac"].astype(np.float64)


def _filler(rng, n, elements):
    lens = rng.uniform(3.5, 7.0, 3)
    ang = rng.uniform(75, 105, 3)
    return cc.cell(*lens, *ang), rng.choice(elements, size=n), rng.uniform(0, 1, (n, 3))


@functools.lru_cache(maxsize=None)
def _build():
    """(structures: name -> dict, the set's names in original order, the samples' names in batch order)."""
    st = dict(G.crystals())
    refs = dict(M.references())
    st.update({name: refs[name] for name in refs})
    case = {c["name"]: c["sample"] for c in M.cases()}
    rng = np.random.default_rng(20261022)
    st["rutile_twin"] = M._structure(*_raw(st["rutile"]))
    assert all(np.array_equal(st["rutile"][f], st["rutile_twin"][f]) for f in ("lattice", "types", "frac"))
    st["quartz_d002"] = M._structure(*M.displaced(_raw(st["quartz"]), 0.02, 500)[0])
    st["cscl_flat"] = M._structure([[4.1, 0, 0], [0, 4.1, 0], [4.1, 4.1, 0]], st["cscl"]["types"], st["cscl"]["frac"])
    in_set = list(refs) + ["rutile_twin", "quartz_d002", "cscl_flat"]
    for name in G.STRUCTURES:
        in_set += [f"{name}_d005", f"{name}_strain30"]
    fill_elements = (np.array([3, 9, 11, 17]), np.array([12, 16, 34]), np.array([13, 15, 31, 33]), np.array([19, 35, 53]),
                     np.array([4, 7, 5]))
    k = 0
    while len(in_set) < 70:
        n = (4, 6, 7, 8, 9, 11)[k % 6]
        st[f"filler{k}"] = M._structure(*_filler(rng, n, fill_elements[k % 5]))
        in_set.append(f"filler{k}")
        k += 1
    # the samples
    samples = []
    for s, name in enumerate(("simple_cubic",) + tuple(G.STRUCTURES)):
        base = _raw(st[name])
        st[f"{name}_again"] = M._structure(*sc._variant(base, rng))
        samples.append(f"{name}_again")
        if name != "quartz":  # (0.05 A from quartz is as far from quartz_d002, within GAP: the set would have no clear best)
            st[f"{name}_d005b"] = M._structure(*sc._variant(M.displaced(base, 0.05, 400 + s)[0], rng))
            samples.append(f"{name}_d005b")
        if name == "simple_cubic":
            st["sc1_variant"] = M._structure(*sc._variant(base, rng))
            samples += ["sc1_variant", "sc1_scale11"]
            continue
        samples += [f"{name}_variant", f"{name}_moved1", f"{name}_scale09" if f"{name}_scale09" in st else f"{name}_scale11"]
        if f"{name}_strain5" in st:
            samples.append(f"{name}_strain5")
    st["quartz_d002_variant"] = M._structure(*sc._variant(_raw(st["quartz_d002"]), rng))
    st["thin_sample"] = case["thin"]
    st["cs_cs"] = case["composition"]
    for name in ("sc_63", "sc_64", "sc_65", "sc_256"):
        st[f"{name}_moved"] = case[f"{name}_d005"]
    samples += ["quartz_d002_variant", "quartz_mirror", "rutile_exchanged", "thin_sample", "cs_cs", "p1_three", "zero_volume",
                "sc_63_moved", "sc_64_moved", "sc_65_moved", "sc_256_moved"]
    k = 0
    while len(samples) < 65:
        L, types, frac = _raw(st[f"filler{k}"])
        st[f"other{k}"] = M._structure(L, types + 40, frac)
        samples.append(f"other{k}")
        k += 1
    assert len(in_set) == 70 and len(set(in_set)) == 70 and len(samples) == 65 and len(set(samples)) == 65
    in_set = [in_set[k] for k in np.random.default_rng(7).permutation(len(in_set))]
    samples = [samples[k] for k in np.random.default_rng(8).permutation(len(samples))]
    return st, tuple(in_set), tuple(samples)


def structures():
    return _build()[0]


def reference_names():
    return _build()[1]


def pool():
    return _build()[2]


def usable(name) -> bool:
    """Has the structure a reduced cell?"""
    return M.reduced(structures()[name]["lattice"]) is not None


@functools.lru_cache(maxsize=None)
def pair(sample, ref, dtype_name="float64"):
    """The restatement's record of `sample` against `ref` (the reference side). Shared: do not modify."""
    dt = np.float32 if dtype_name == "float32" else np.float64
    return M.restate(structures()[sample], structures()[ref], dt)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (sample names in batch order, exclusion mask as a bool array or None)."""
    p = pool()
    mask = np.zeros(33, dtype=bool)
    mask[[1, 8, 20, 31]] = True
    out = {f"first{B}": (p[:B], None) for B in (1, 2, 33, 65)}
    out["excluded"] = (p[:33], mask)
    return out


@functools.lru_cache(maxsize=None)
def expected(batch, dtype_name="float64", names=None):
    """Per sample of a batch a dict: key, lo, cands (original indices in sorted order), records (the restatement's
    per candidate), n_candidates, n_matched, known, ref (original index, -1), rms, max_dist, flags. `names` = the
    set's names in another original order (default reference_names())."""
    names = reference_names() if names is None else names
    st = structures()
    structs = [st[r] for r in names]
    order, _ = sort_set(structs)
    samples, mask = batches()[batch]
    out = []
    for g, s in enumerate(samples):
        gone, flat = bool(mask is not None and mask[g]), not usable(s)
        rec = dict(key=key_of(st[s]["types"]), lo=0, cands=[], records=[], n_candidates=0, n_matched=0, known=False,
                   ref=-1, rms=0.0, max_dist=0.0, flags=(EXCLUDED if gone else 0) | (M.NO_LATTICE if flat else 0))
        if not gone and not flat:
            at = candidates_of(st[s], structs, order)
            rec["lo"] = at[0] if at else 0
            rec["cands"] = [order[p] for p in at]
            rec["records"] = [pair(s, names[r], dtype_name) for r in rec["cands"]]
            rec["n_candidates"] = len(at)
            hits = sorted((r["rms"], o) for r, o in zip(rec["records"], rec["cands"]) if r["matched"])
            rec["n_matched"] = len(hits)
            if hits:
                win = rec["records"][rec["cands"].index(hits[0][1])]
                rec.update(known=True, ref=hits[0][1], rms=win["rms"], max_dist=win["max_dist"], flags=win["flags"])
        out.append(rec)
    return out


def float32_error():
    """The largest |float32 - float64| of rms and max_dist over every candidate pair of the largest batch."""
    worst = 0.0
    for a, c in zip(expected("first65", "float32"), expected("first65", "float64")):
        for ra, rc in zip(a["records"], c["records"]):
            worst = max(worst, abs(ra["rms"] - rc["rms"]), abs(ra["max_dist"] - rc["max_dist"]))
    return worst


def packed_set(names=None):
    """(natoms, types, frac, lattices) of the set in its original order."""
    return M.packed([structures()[r] for r in (reference_names() if names is None else names)])


def packed(batch):
    """(natoms, types int64 [N], frac float32 [N,3], lattices float32 [B,3,3], mask or None) of a batch."""
    names, mask = batches()[batch]
    return M.packed([structures()[c] for c in names]) + (mask,)
