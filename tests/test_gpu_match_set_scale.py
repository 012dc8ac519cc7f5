"""The reference-set search on the device at the scale where a block of k_set_pairs runs several pairs and
k_set_offsets scans more than one round (chemeleon_amd.match_set, csrc/match.hip), on the cases of
tests/match_set_scale_cases.py: 300 samples, 2 061 pairs, under both pairings.

The pair kernel's grid is min(num_pairs_max, 3 x compute units), 768 blocks on an MI355X, and block b runs pairs b,
b + grid, b + 2 grid of the list: from its second pair on, match_block starts with the LDS of the pair before. The
tests reach that by pair count alone and assert it (P >= 2 grid + 1, and at least 50 blocks see each of: a collided
pair then a clean match, a match then an early exit, an early exit then a match, a match then an unmatched pair).
Checked: every record and every launched pair against the float64 restatement (integers exactly; rms and max_dist
within 16 times the float32 restatement's own error, 1.1e-5, below 1e-3 stol); the same samples in chunks of 16, where
no block runs a second pair, byte for byte, and each winner against match_states (k_match, one block per crystal);
the batch reversed, permuted, and run twice through one plan on dirty buffers; first[] against a cumulative sum for
B = 256, 257, 300 and 513 and with the whole first round excluded; and one graph replay on a permuted state."""

import numpy as np
import pytest
import torch

from chemeleon_amd import Match, MatchSet, MatchSetReport, Reference, ReferenceSet, match_set_states, match_states
from chemeleon_amd.cell import cell_plan
from chemeleon_amd.match import MATCH_CELL_ANGLE_TOLERANCE, MATCH_CELL_SYMPREC
from chemeleon_amd.match_set import match_set_plan
from tests import match_cases as M
from tests import match_set_cases as S
from tests import match_set_scale_cases as C

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
BLOCKS_PER_CU = 3  # CHM_MATCH_SET_BLOCKS_PER_CU (include/chemeleon_hip.h)
CHUNK = 16
pairings = pytest.mark.parametrize("pairing", C.PAIRINGS)


def on_device(names):
    nat, types, frac, lat = C.packed(names)
    return nat, torch.from_numpy(types).to(DEV), torch.from_numpy(frac).to(DEV), torch.from_numpy(lat).to(DEV)


def take(state, index):
    """The crystals `index` of a device state, in that order."""
    nat, a, x, lat = state
    first = np.concatenate([[0], np.cumsum(nat)])
    nodes = torch.from_numpy(np.concatenate([np.arange(first[g], first[g + 1]) for g in index])).to(DEV)
    return [nat[g] for g in index], a[nodes], x[nodes], lat[torch.as_tensor(np.asarray(index), device=DEV)]


@pytest.fixture(scope="module")
def refset():
    return ReferenceSet.from_arrays(*C.packed_set())


@pytest.fixture(scope="module")
def state():
    return on_device(C.batch()[0])


@pytest.fixture(scope="module")
def big(refset, state):
    """pairing -> the MatchSetReport of the whole masked batch, run once."""
    return {p: match_set_states(*state, MatchSet(refset, pairing=p), C.batch()[1]) for p in C.PAIRINGS}


@pytest.fixture(scope="module")
def gate():
    g = C.gate()
    assert g < 1e-3 * M.STOL
    return g


def grid_of(refset, nat):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, min(match_set_plan(nat, refset, DEV).num_pairs_max, BLOCKS_PER_CU * cus)


def sample_slices(rep, g):
    a = int(rep.first[g])
    return rep.records[g, :40], rep.pair_records[a:a + int(rep.n_candidates[g])]


def device_mask(mask):
    return None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).to(DEV)


def raw_run(state, refset, pairing, ex, bufs, cell_rec=None):
    """The cell pass and the search enqueued through the cached plans into (out, pair records, workspace); no host
    wait. Returns what must stay alive until the stream is through."""
    nat, a, x, lat = state
    plan, cells = match_set_plan(nat, refset, DEV), cell_plan(nat, DEV)
    ra, rx, rlat, rrec = refset.on(DEV)
    if cell_rec is None:
        cell_rec = torch.empty(len(nat) * 128, dtype=torch.uint8, device=DEV)
    cells.run(lat, None, MATCH_CELL_SYMPREC, MATCH_CELL_ANGLE_TOLERANCE, cell_rec)
    plan.run(cell_rec, a, x, lat, rrec, ra, rx, rlat, ex, M.LTOL, M.STOL, M.ANGLE_TOL, *bufs, pairing)
    return cell_rec, ex, plan, cells


def buffers(refset, nat, fill):
    plan = match_set_plan(nat, refset, DEV)
    return (torch.full((48 * len(nat),), fill, dtype=torch.uint8, device=DEV),
            torch.full((16 * plan.num_pairs_max,), fill, dtype=torch.uint8, device=DEV),
            torch.full((plan.workspace_bytes,), fill, dtype=torch.uint8, device=DEV))


@pairings
def test_every_block_runs_several_pairs_of_mixed_kinds(refset, state, big, pairing):
    rep = big[pairing]
    cus, grid = grid_of(refset, state[0])
    P = len(rep.pair_records)
    seen = C.transitions(grid)
    print(f"{pairing}: P = {P}, {cus} compute units, grid = {grid}, pairs per block {P // grid} to {-(-P // grid)}; "
          f"blocks that see each transition: {seen}")
    assert P == len(C.kinds()) >= 2 * BLOCKS_PER_CU * cus + 1
    assert grid == BLOCKS_PER_CU * cus and P >= 2 * grid + 1
    assert min(seen.values()) >= 50, seen


@pairings
def test_records_and_pairs_against_the_float64_restatement(big, gate, pairing):
    rep, want = big[pairing], C.expected(pairing)
    names, samples = C.reference_names(), C.batch()[0]
    assert len(rep) == len(want) == C.B
    worst = 0.0
    for g, (s, w) in enumerate(zip(samples, want)):
        assert int(rep.key[g]) == w["key"], s
        got = (bool(rep.known[g]), int(rep.ref[g]), int(rep.n_candidates[g]), int(rep.n_matched[g]), int(rep.flags[g]))
        assert got == (w["known"], w["ref"], w["n_candidates"], w["n_matched"], w["flags"]), (s, got)
        assert (w["n_candidates"] == 0 or int(rep.lo[g]) == w["lo"]) and (rep.position[g] >= 0) == w["known"]
        refs, matched, rms = rep.candidates(g)
        assert refs.tolist() == w["cands"], s
        first = int(rep.first[g])
        for k, r in enumerate(w["records"]):
            at = first + k
            assert bool(matched[k]) == bool(r["matched"]) and rep.pair_flags[at] == r["flags"], (s, names[refs[k]])
            assert rep.pair_n_assigned[at] == (r["n_assigned"] if pairing == "assignment" else 0), (s, names[refs[k]])
            err = max(abs(float(rms[k]) - r["rms"]), abs(float(rep.pair_max_dist[at]) - r["max_dist"]))
            assert err <= gate, (s, names[refs[k]], err)
            worst = max(worst, err)
        err = max(abs(float(rep.rms[g]) - w["rms"]), abs(float(rep.max_dist[g]) - w["max_dist"]))
        assert err <= gate, (s, err)
        worst = max(worst, err)
        if w["known"]:
            at = first + int(rep.position[g]) - int(rep.lo[g])
            np.testing.assert_array_equal(rep.records[g, :12], rep.pair_records[at, :12])
            assert rep.pair_ref[at] == w["ref"] and rep.pair_sample[at] == g
        else:
            assert not rep.records[g, :8].any() and rep.ref[g] == -1
    assert rep.first.tolist() == np.concatenate([[0], np.cumsum(rep.n_candidates)[:-1]]).tolist()
    assert rep.n_known == sum(w["known"] for w in want) and len(rep.pair_records) == rep.n_candidates.sum()
    print(f"{pairing}: largest device error against float64: {worst:.3e}, gate {gate:.3e}")


@pairings
def test_one_pair_per_block_gives_the_same_bytes(refset, state, big, pairing):
    """The same samples in chunks of 16 (fewer pairs than blocks: no block runs a second pair), and every winner
    against match_states (k_match: one block per crystal)."""
    rep, mask = big[pairing], C.batch()[1]
    search = MatchSet(refset, pairing=pairing)
    for lo in range(0, C.B, CHUNK):
        index = list(range(lo, min(lo + CHUNK, C.B)))
        part = take(state, index)
        _, grid = grid_of(refset, part[0])
        small = match_set_states(*part, search, mask[index])
        assert len(small.pair_records) <= grid and len(small.pair_records) <= CHUNK * 9
        for k, g in enumerate(index):
            for got, want in zip(sample_slices(small, k), sample_slices(rep, g)):
                np.testing.assert_array_equal(got, want, err_msg=f"sample {g}")
    ref = Reference.from_arrays(*C.packed_set())
    single = match_states(*state, Match(ref, ref_of=rep.ref.tolist(), pairing=pairing))
    known = np.flatnonzero(rep.known)
    assert len(known) > 130 and single.matched[known].all() and not single.matched[~rep.known].any()
    np.testing.assert_array_equal(rep.records[known, :8], single.records[known, :8])  # rms, max_dist
    np.testing.assert_array_equal(rep.flags[known], single.flags[known])


@pairings
def test_bytes_do_not_depend_on_the_order_or_on_what_the_buffers_held(refset, state, big, pairing):
    rep, mask = big[pairing], C.batch()[1]
    search = MatchSet(refset, pairing=pairing)
    for perm in (np.arange(C.B)[::-1].copy(), np.random.default_rng(31).permutation(C.B)):
        other = match_set_states(*take(state, perm.tolist()), search, mask[perm])
        assert len(other.pair_records) == len(rep.pair_records)
        for k, g in enumerate(perm.tolist()):
            for got, want in zip(sample_slices(other, k), sample_slices(rep, g)):
                np.testing.assert_array_equal(got, want, err_msg=f"sample {g}")
    # twice through one plan and one set of buffers, filled with a pattern before the first run and holding the first
    # run's winner words and match counts before the second
    bufs = buffers(refset, state[0], 0xAB)
    ex = device_mask(mask)
    held = raw_run(state, refset, pairing, ex, bufs)
    once = [t.cpu().numpy().copy() for t in bufs]
    bufs[0].fill_(0x5C)
    held = raw_run(state, refset, pairing, ex, bufs)
    twice = [t.cpu().numpy() for t in bufs]
    del held
    for a, b in zip(once, twice):
        np.testing.assert_array_equal(a, b)
    got = MatchSetReport(twice[0], twice[1], refset.order)
    np.testing.assert_array_equal(got.records, rep.records)
    np.testing.assert_array_equal(got.pair_records, rep.pair_records)
    P = len(rep.pair_records)
    assert (twice[1][16 * P:] == 0xAB).all() and 16 * P < len(twice[1])  # (the list is compact: its tail is left alone)


def test_the_scan_of_the_candidate_counts(refset):
    """first[] = the exclusive cumulative sum of n_candidates over one full round (256), one sample more, a partial
    second round (300), two rounds and one sample (513), and with every sample of the first round excluded."""
    runs = [(n, None) for n in (256, 257, 300, 513)] + [(n, np.arange(n) < 256) for n in (300, 513)]
    for n, mask in runs:
        st = on_device(C.scan_batch(n))
        bufs = buffers(refset, st[0], 0xAB)
        held = raw_run(st, refset, "nearest", device_mask(mask), bufs)
        out, prec, ws = (t.cpu().numpy() for t in bufs)
        del held
        rep = MatchSetReport(out, prec, refset.order)
        first = ws[16 * n + 12 * n:16 * n + 12 * n + 4 * (n + 1)].view(np.int32)  # behind keys, winners, lo, cnt, n_matched
        cnt = ws[16 * n + 4 * n:16 * n + 8 * n].view(np.int32)
        np.testing.assert_array_equal(cnt, rep.n_candidates)
        np.testing.assert_array_equal(first, np.concatenate([[0], np.cumsum(rep.n_candidates)]))
        np.testing.assert_array_equal(rep.first, first[:-1])
        P = int(first[n])
        assert P == len(rep.pair_records) and P > 9 * 9
        written = prec.reshape(-1, 16)
        assert (written[P:] == 0xAB).all() and not (written[:P] == 0xAB).all(axis=1).any()
        if mask is None:
            assert n < 300 or rep.n_candidates[256:].any()
        else:  # every candidate sits behind the carry
            assert not rep.n_candidates[:256].any() and (first[:257] == 0).all() and P > 0
            assert (rep.flags[:256] & S.EXCLUDED).all() and not (rep.flags[256:] & S.EXCLUDED).any()


@pairings
def test_a_replayed_graph_at_this_scale(refset, state, big, pairing):
    """Captured on the batch; the state is overwritten in place with a permutation of it that keeps every position's
    atom count; the replay equals an eager run on the permuted state (and back)."""
    mask = C.batch()[1]
    perm = C.size_preserving_permutation(21)
    second = take(state, perm.tolist())
    assert second[0] == state[0] and not torch.equal(second[1], state[1])
    want = [big[pairing], match_set_states(*second, MatchSet(refset, pairing=pairing), mask)]
    assert not np.array_equal(want[0].n_candidates, want[1].n_candidates)  # (so the pair list is laid out anew)
    nat = state[0]
    a, x, lat = (t.clone() for t in state[1:])
    bufs = buffers(refset, nat, 0x11)
    ex, cell_rec = device_mask(mask), torch.zeros(C.B * 128, dtype=torch.uint8, device=DEV)
    held = raw_run((nat, a, x, lat), refset, pairing, ex, bufs, cell_rec)  # (the plans exist before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            held = raw_run((nat, a, x, lat), refset, pairing, ex, bufs, cell_rec)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 0):
        for t, src in zip((a, x, lat), (state, second)[k][1:]):
            t.copy_(src)
        bufs[0].fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        got = MatchSetReport(bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), refset.order)
        np.testing.assert_array_equal(got.records, want[k].records)
        np.testing.assert_array_equal(got.pair_records, want[k].pair_records)
    del held
