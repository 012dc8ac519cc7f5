"""The cases of grouping by matching on the CPU (tests/match_group_cases.py): the float64 restatement of
tests/match_cases.py over every pair of equal size and the plain leader rule give the stated groups, every pair
keeps match_cases' margins so that float32 arithmetic decides nothing differently, the float32 restatement yields
the same match matrix and groups, and MatchDedup validates its arguments without a device.

Measured here (float32 restatement against float64 over every searched pair of every batch): 8.7e-7 (the largest of
rms and max_dist in A). The gate of tests/test_gpu_match_group.py is 16 times that, 1.4e-5, and must stay below
1e-3 stol = 3e-4."""

import numpy as np
import pytest

from chemeleon_amd import MatchDedup
from chemeleon_amd.match_group import pair_table
from tests import match_cases as M
from tests import match_group_cases as G


def groups_of(batch):
    names, _ = G.batches()[batch]
    e = G.expected(batch)
    return {names[r]: sorted(names[g] for g in np.flatnonzero(e["group"] == r)) for r in np.flatnonzero(e["count"] > 0)}


def test_the_leader_rule_gives_the_stated_groups():
    names, _ = G.batches()["first65"]
    e = G.expected("first65")
    assert len(names) == 65
    # every disguised copy is with its structure, every non-duplicate on its own
    for s in G.STRUCTURES:
        same = [g for g, n in enumerate(names) if n == s or n.startswith(s + "_") and
                n[len(s) + 1:] in ("variant", "d005", "scale09", "scale11", "strain5", "mirror")]
        assert len(same) >= 4 and len(set(e["group"][same].tolist())) == 1, s
        lead = int(e["group"][same[0]])
        assert lead == min(same) and e["count"][lead] == len(same), s
        for kind in ("strain30", "moved1", "exchanged"):
            if s + "_" + kind in names:
                g = names.index(s + "_" + kind)
                assert e["group"][g] == g and e["count"][g] == 1, (s, kind)
    assert e["group"][names.index("quartz_mirror")] == e["group"][names.index("quartz")]
    assert names.index("rutile_exchanged") >= 0 and "rutile_exchanged" in groups_of("first65")
    # the representatives are spread over the batch, not its first crystals
    reps = np.flatnonzero(e["count"] > 0)
    assert reps.max() > 60 and not np.array_equal(reps, np.arange(len(reps)))
    assert e["count"].sum() == (e["group"] >= 0).sum() == 64


def test_the_chain_is_not_transitive_and_depends_on_the_order():
    assert [G.pair(h, g)["matched"] for h, g in (("chain_a", "chain_b"), ("chain_b", "chain_c"), ("chain_a", "chain_c"),
                                                  ("chain_b", "chain_a"))] == [1, 1, 0, 1]
    assert G.expected("chain_abc")["group"].tolist() == [0, 0, 2]
    assert G.expected("chain_abc")["count"].tolist() == [2, 0, 1]
    assert G.expected("chain_bac")["group"].tolist() == [0, 0, 0]
    assert G.expected("chain_bac")["count"].tolist() == [3, 0, 0]


def test_sizes_exclusion_degenerate_and_thin():
    assert sorted(len(G.batches()[b][0]) for b in G.batches()) == [1, 2, 3, 3, 31, 32, 33, 33, 65]
    names, _ = G.batches()["first65"]
    sizes = [len(G.crystals()[n]["types"]) for n in names]
    assert sizes.count(3) == 1 and sizes.count(65) == 2 and sizes.count(1) == 2  # once; one pair; one pair
    assert [(h, g) for h, g in G.pairs_of(names) if sizes[g] in (1, 65)] == [(2, 29), (26, 40)]
    e = G.expected("first65")
    assert e["matched"][[G.pairs_of(names).index(p) for p in ((2, 29), (26, 40))]].all()
    # the zero-volume lattice: group -1, never a leader, nobody's leader
    z = names.index("zero_volume")
    assert not G.usable("zero_volume") and e["group"][z] == -1 and e["count"][z] == 0 and not (e["group"] == z).any()
    assert all(r is None for (h, g), r in zip(e["pairs"], e["records"]) if z in (h, g))
    # the thin leader: the pair sets THIN, both stay groups of their own
    a, b = names.index("thin_a"), names.index("thin_b")
    assert G.pair("thin_a", "thin_b")["flags"] == M.THIN and not G.pair("thin_a", "thin_b")["matched"]
    assert a < b and e["group"][a] == a and e["group"][b] == b and e["count"][a] == e["count"][b] == 1
    # the exclusion mask takes out a representative (its members regroup under the next one) and a member
    names33, mask = G.batches()["excluded"]
    free, ex = G.expected("first33"), G.expected("excluded")
    assert mask.sum() == 3 and free["count"][0] > 1 and free["group"][17] == 7
    assert (ex["group"][mask] == -1).all() and (ex["count"][mask] == 0).all() and not np.isin(ex["group"], np.flatnonzero(mask)).any()
    assert ex["group"][10] == 10 and ex["group"][21] == 10 and free["group"][10] == free["group"][21] == 0
    assert ex["count"][7] == free["count"][7] - 1


def test_every_pair_keeps_its_margins():
    searched = 0
    for b in G.batches():
        names, _ = G.batches()[b]
        e = G.expected(b)
        for (h, g), r in zip(e["pairs"], e["records"]):
            if r is None:
                continue
            for m in ("lattice_margin", "pair_margin", "gap_margin", "thin_margin"):
                assert r[m] >= M.MARGIN, (b, names[h], names[g], m, r[m])
            assert not r["flags"] & M.MANY_MAPPINGS and r["n_mappings"] <= M.MAX_MAPPINGS, (b, names[h], names[g])
            assert not r["flags"] & (M.SIZE | M.NO_LATTICE | M.NO_REFERENCE), (b, names[h], names[g])
            searched += r["flags"] == 0
    assert searched > 200


def test_float32_restatement_gives_the_same_matrix_and_groups():
    for b in G.batches():
        a, c = G.expected(b, "float32"), G.expected(b, "float64")
        assert np.array_equal(a["matched"], c["matched"]), b
        assert np.array_equal(a["group"], c["group"]) and np.array_equal(a["count"], c["count"]), b
        for x, y in zip(a["records"], c["records"]):
            assert (x is None) == (y is None)
            if x is not None:
                assert all(x[f] == y[f] for f in ("flags", "n_mappings", "n_candidates", "n_survivors")), b
    err = G.float32_error()
    print("float32 restatement error over the pairs:", err)
    assert 0 < 16 * err < 1e-3 * M.STOL, err


def test_pair_table_and_arguments():
    names, _ = G.batches()["first33"]
    nat = [len(G.crystals()[n]["types"]) for n in names]
    assert pair_table(nat).tolist() == [list(p) for p in G.pairs_of(names)]
    assert pair_table([4]).shape == (0, 2) and pair_table([2, 3, 2, 2]).tolist() == [[0, 2], [0, 3], [2, 3]]
    d = MatchDedup()
    assert (d.ltol, d.stol, d.angle_tol) == (0.2, 0.3, 5.0)
    for kw in (dict(ltol=0), dict(ltol=1.5), dict(stol=-0.1), dict(stol=float("nan")), dict(angle_tol=31),
               dict(angle_tol="5"), dict(ltol=True)):
        with pytest.raises(ValueError):
            MatchDedup(**kw)
    import torch
    from chemeleon_amd import match_group_states
    s = G.crystals()["cscl"]
    with pytest.raises(RuntimeError, match="HIP device only"):
        match_group_states([2], torch.from_numpy(s["types"]), torch.from_numpy(s["frac"]),
                           torch.from_numpy(s["lattice"][None]))
    with pytest.raises(ValueError, match="chemeleon_amd.MatchDedup"):
        match_group_states([2], None, None, None, "cscl")
    with pytest.raises(ValueError, match="at most 256"):
        match_group_states([257], None, None, None)
