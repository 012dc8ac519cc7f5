"""The cases of the reference-set search check themselves on the CPU (tests/match_set_cases.py): the set and the
samples hold what the GPU tests rely on; every deciding quantity of every candidate pair stays 1e-3 of its bound
away in float64; apart from the deliberate tie the best and the second-best matched rms of a sample differ by at
least 1e-3; no pair sets MANY_MAPPINGS; the float32 restatement gives the same known, ref, n_matched and
n_candidates as float64 (its largest difference in rms / max_dist is printed: the GPU gate is 16 times that); the key
is invariant under permutation, separates every pair of distinct compositions of the cases, and agrees with
chemeleon_amd.match_set.composition_keys and ReferenceSet's sort."""

import numpy as np

from tests import match_cases as M
from tests import match_set_cases as S


def test_the_set_holds_what_the_cases_need():
    st, names = S.structures(), S.reference_names()
    sizes = [len(st[r]["types"]) for r in names]
    assert len(names) == 70 and {1, 2, 63, 64, 65, 256} <= set(sizes)
    order, keys = S.sort_set([st[r] for r in names])
    assert order != list(range(len(names)))
    assert [(sizes[r], k) for r, k in zip(order, keys)] == sorted((sizes[r], k) for r, k in zip(order, keys))
    assert sizes.count(63) == 1 and sizes.count(256) == 1         # sizes with a single reference
    a, b = (names.index(t) for t in S.TWINS)
    assert abs(order.index(a) - order.index(b)) == 1                # the twins are neighbours in the sorted set
    assert not S.usable("cscl_flat") and "cscl_flat" in names
    assert S.key_of(st["quartz"]["types"]) == S.key_of(st["quartz_d002"]["types"])


def test_the_samples_hold_what_the_cases_need():
    st, names, pool = S.structures(), S.reference_names(), S.pool()
    structs = [st[r] for r in names]
    order, _ = S.sort_set(structs)
    sizes = {len(s["types"]) for s in structs}
    assert len(pool) == 65 and [len(b[0]) for b in S.batches().values()] == [1, 2, 33, 65, 33]
    assert len(st["p1_three"]["types"]) not in sizes                # a size the set does not hold
    for name in ("cs_cs", "other0", "other1", "other2", "other3"):            # a size it holds, a composition it does not
        assert len(st[name]["types"]) in sizes and S.candidates_of(st[name], structs, order) == []
    want = {r["ref"] for r in S.expected("first65")}
    assert {names.index("quartz"), names.index("quartz_d002"), min(names.index(t) for t in S.TWINS)} <= want
    by = dict(zip(pool, S.expected("first65")))
    assert by["quartz_d002_variant"]["ref"] == names.index("quartz_d002") and by["quartz_d002_variant"]["n_matched"] >= 2
    assert by["quartz_variant"]["ref"] == names.index("quartz") and by["quartz_mirror"]["known"]
    ex = by["rutile_exchanged"]
    assert ex["n_candidates"] >= 2 and not ex["known"] and ex["n_matched"] == 0
    assert by["thin_sample"]["n_candidates"] == 1 and by["thin_sample"]["records"][0]["flags"] == M.THIN
    assert by["zero_volume"]["flags"] == M.NO_LATTICE and by["zero_volume"]["n_candidates"] == 0
    flat = [r for r, o in zip(by["cscl_variant"]["records"], by["cscl_variant"]["cands"]) if names[o] == "cscl_flat"]
    assert len(flat) == 1 and flat[0]["flags"] == M.NO_LATTICE and not flat[0]["matched"]
    for name in ("sc_63_moved", "sc_64_moved", "sc_65_moved", "sc_256_moved", "simple_cubic_again", "cscl_again"):
        assert by[name]["known"], name
    known = sum(r["known"] for r in by.values())
    assert 30 <= known <= 55 and sum(r["n_matched"] >= 2 for r in by.values()) >= 8
    masked = S.expected("excluded")
    assert [r["flags"] & S.EXCLUDED != 0 for r in masked] == S.batches()["excluded"][1].tolist()
    assert any(r["known"] for r, m in zip(S.expected("first33"), S.batches()["excluded"][1]) if m)


def test_margins_gaps_and_the_float32_restatement():
    names = S.reference_names()
    twins = {names.index(t) for t in S.TWINS}
    f64, f32 = S.expected("first65"), S.expected("first65", "float32")
    pairs = 0
    for s, a, b in zip(S.pool(), f64, f32):
        for key in ("key", "lo", "cands", "n_candidates", "n_matched", "known", "ref", "flags"):
            assert a[key] == b[key], (s, key)
        for r, r32, o in zip(a["records"], b["records"], a["cands"]):
            pairs += 1
            assert not r["flags"] & M.MANY_MAPPINGS and not r32["flags"] & M.MANY_MAPPINGS, (s, names[o])
            assert (r["matched"], r["flags"]) == (r32["matched"], r32["flags"]), (s, names[o])
            for m in ("lattice_margin", "pair_margin", "gap_margin", "thin_margin"):
                assert r[m] >= M.MARGIN, (s, names[o], m, r[m])
            if r["flags"] == 0:  # the score against its bound: rms <= stol decides whether a survivor counts
                assert all(abs(c[2] - M.STOL) >= M.MARGIN * M.STOL for c in r["counting"]), (s, names[o])
        hits = sorted((r["rms"], o) for r, o in zip(a["records"], a["cands"]) if r["matched"])
        if len(hits) >= 2:
            if {hits[0][1], hits[1][1]} == twins:
                assert hits[0][0] == hits[1][0] and a["ref"] == min(twins)
                hits = hits[1:]
            if len(hits) >= 2:
                assert hits[1][0] - hits[0][0] >= S.GAP, (s, hits[:2])
    err = S.float32_error()
    print(f"{pairs} candidate pairs; largest |float32 - float64| of rms / max_dist: {err:.3e}; gate {16 * err:.3e}")
    assert 16 * err < 1e-3 * M.STOL


def test_another_original_order_gives_the_same_winners():
    names = S.reference_names()
    other = tuple(names[k] for k in np.random.default_rng(11).permutation(len(names)))
    for a, b in zip(S.expected("first33"), S.expected("first33", "float64", other)):
        assert (a["key"], a["n_candidates"], a["n_matched"], a["known"]) == (b["key"], b["n_candidates"], b["n_matched"], b["known"])
        if a["known"] and names[a["ref"]] not in S.TWINS:
            assert other[b["ref"]] == names[a["ref"]]
        elif a["known"]:
            assert b["ref"] == min(other.index(t) for t in S.TWINS)


def test_the_key():
    st = S.structures()
    rng = np.random.default_rng(3)
    comps = {}
    for name, s in st.items():
        t = s["types"]
        assert S.key_of(t) == S.key_of(rng.permutation(t)), name
        comps.setdefault(tuple(sorted(t.tolist())), S.key_of(t))
    assert len(set(comps.values())) == len(comps) > 40               # distinct compositions, distinct keys
    assert S.key_of([0]) == 0x5692161d100b05e5 and S.key_of([-1]) == S.key_of([0xffffffff])  # splitmix64's mix of 1
    from chemeleon_amd.match_set import ReferenceSet, composition_keys
    nat, types, frac, lat = S.packed_set()
    want = [S.key_of(st[r]["types"]) for r in S.reference_names()]
    assert [int(k) for k in composition_keys(nat, types)] == want
    rs = ReferenceSet.from_arrays(nat, types, frac, lat)
    order, keys = S.sort_set([st[r] for r in S.reference_names()])
    assert rs.order.tolist() == order and [int(k) for k in rs.keys] == keys
    assert list(rs.natoms) == [nat[r] for r in order]
    np.testing.assert_array_equal(rs.lattices, lat[order])
