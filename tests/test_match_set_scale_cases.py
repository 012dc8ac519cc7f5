"""The cases of the reference-set search at scale check themselves on the CPU (tests/match_set_scale_cases.py): B
and P (P >= 2 x 768 + 200, so on the 768 blocks of an MI355X every block runs two pairs and some three), the
histograms of n_candidates and n_matched under both pairings, the number of pairs of each kind and the blocks of a
grid of 768 that see each transition of kinds, the zero-candidate run across sample 256 and the mask on both sides
of it; float32 and float64 restate every pair and sample to the same matched, flags, counts, known and ref, with
every deciding quantity MARGIN of its bound away; and the float32 restatement's largest rms / max_dist error against
float64, which is printed with the time the restatements took: the GPU gate is 16 times that error."""

import collections
import itertools

import numpy as np

from tests import assign_cases as A
from tests import match_cases as M
from tests import match_set_cases as S
from tests import match_set_scale_cases as C


def hist(values):
    return dict(sorted(collections.Counter(values).items()))


def test_the_batch_and_its_pair_list_are_pinned():
    names, mask = C.batch()
    assert len(names) == C.B == 300 and len(C.reference_names()) == 99 and mask.sum() == len(C.MASKED)
    near, asg = C.expected("nearest"), C.expected("assignment")
    P = sum(r["n_candidates"] for r in near)
    assert P == 2061 and C.P_FLOOR == 1736 <= P <= 2400 and P == sum(r["n_candidates"] for r in asg) == len(C.kinds())
    assert hist(r["n_candidates"] for r in near) == {0: 71, 9: 229} == hist(r["n_candidates"] for r in asg)
    assert hist(r["n_matched"] for r in near) == {0: 162, 1: 34, 2: 1, 3: 3, 4: 11, 5: 63, 6: 26}
    assert hist(r["n_matched"] for r in asg) == {0: 90, 1: 34, 2: 1, 3: 2, 4: 15, 5: 132, 6: 26}
    sizes = hist(len(C.structures()[s]["types"]) for s in names)
    assert set(sizes) == {1, 2, 3, 4, 5, 6, 7, 8} and sizes[2] + sizes[4] > 150 > sizes[8] > 0
    # every bucket: 9 references, one of them without a reduced cell, one thin
    for refs in C._build()[2].values():
        assert len(refs) == 9 and sum(not C.usable(r) for r in refs) == 1
    # the candidate counts around the scan's round boundary, and the mask on both sides of it
    cnt = np.array([r["n_candidates"] for r in C.expected("nearest", "float64", False)])
    assert not cnt[250:262].any() and cnt[240:250].any() and cnt[262] and {len(C.structures()[s]["types"]) for s in names[250:262]} > {6, 7}
    assert sum(C.usable(s) for s in names[250:262]) == 8  # (four of the run have no reduced cell)
    assert mask[:256].sum() >= 3 and mask[256:].sum() >= 3 and cnt[mask].sum() > 40  # (the mask takes candidates away)
    flags = [r["flags"] for r in near]
    assert flags.count(S.EXCLUDED) == 7 and flags.count(M.NO_LATTICE) == 10 and flags.count(S.EXCLUDED | M.NO_LATTICE) == 2


def test_the_kinds_of_pair_and_what_a_block_sees_in_sequence():
    kinds = C.kinds()
    count = collections.Counter(kinds)
    print("pairs per kind:", dict(count))
    assert dict(count) == {C.UNMATCHED: 680, C.MATCHED: 540, C.EARLY: 458, C.COLLIDED: 383}
    assert min(count.values()) >= 100
    seen = C.transitions(768)
    print("blocks of a grid of 768 that see each transition:", seen)
    assert seen == {(C.COLLIDED, C.MATCHED): 68, (C.MATCHED, C.EARLY): 72, (C.EARLY, C.MATCHED): 89,
                    (C.MATCHED, C.UNMATCHED): 115}
    assert min(seen.values()) >= 50
    # the order is mixed: no kind comes in runs much longer than one sample's nine candidates
    assert max(len(list(g)) for _, g in itertools.groupby(kinds)) <= 12
    # the collided pairs do phase-B work, and the nearest rule drops what the assignment solves
    near, asg = C.expected("nearest"), C.expected("assignment")
    solved = [(n, a) for sn, sa in zip(near, asg) for n, a in zip(sn["records"], sa["records"]) if a["n_assigned"]]
    assert len(solved) == count[C.COLLIDED] and sum(a["matched"] and not n["matched"] for n, a in solved) > 150
    assert sum(a["collided"] for n, a in solved) > 150  # (the winner itself is a solved candidate)
    early = collections.Counter(a["flags"] for sa in asg for a in sa["records"] if a["flags"])
    assert early == {M.NO_LATTICE: 229, M.THIN: 229}


def test_float32_and_float64_agree_and_the_gate():
    pairs = 0
    for pairing, fields, margins in (("nearest", M.INT_FIELDS, C.NEAR_MARGINS), ("assignment", A.INT_FIELDS, C.ASSIGN_MARGINS)):
        f64, f32 = C.expected(pairing), C.expected(pairing, "float32")
        for s, a, b in zip(C.batch()[0], f64, f32):
            for key in ("key", "lo", "cands", "n_candidates", "n_matched", "known", "ref", "flags"):
                assert a[key] == b[key], (pairing, s, key)
            for r, r32, o in zip(a["records"], b["records"], a["cands"]):
                pairs += 1
                assert all(r[f] == r32[f] for f in fields), (pairing, s, o)
                assert not r["flags"] & (M.MANY_MAPPINGS | A.MANY_ASSIGNMENTS)
                assert all(r[m] >= C.MARGIN for m in margins), (pairing, s, o)
            for recs in (a["records"], b["records"]):
                assert C._winner_gap(recs) >= C.GAP, (pairing, s)
    errs = {p: C.float32_error(p) for p in C.PAIRINGS}
    print(f"{pairs} restated pairs; the float64 restatements took {C.SECONDS['float64']:.1f} s, the float32 ones "
          f"{C.SECONDS['float32']:.1f} s; largest |float32 - float64| of rms / max_dist: {errs}; gate {C.gate():.3e}")
    assert pairs == 2 * 2061
    assert 0 < C.gate() == 16 * max(errs.values()) < 1e-3 * M.STOL
    assert C.GAP > 8 * C.gate()  # (two device values, each within the gate, cannot exchange a winner)


def test_the_derived_batches():
    perm = C.size_preserving_permutation(21)
    names, st = C.batch()[0], C.structures()
    assert sorted(perm.tolist()) == list(range(C.B)) and (perm != np.arange(C.B)).sum() > 250
    assert [len(st[names[k]]["types"]) for k in perm] == [len(st[s]["types"]) for s in names]
    for n in (256, 257, 300, 513):
        got = C.scan_batch(n)
        assert len(got) == n and got[:min(n, C.B)] == names[:min(n, C.B)] and got[C.B:] == names[:max(0, n - C.B)]
