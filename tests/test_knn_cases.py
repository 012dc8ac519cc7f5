"""The cases of the radius-graph unit tests (tests/knn_cases.py) on the CPU: the float64 reference written from the
definition equals the oracle (oracle/knn_oracle.py, the torch fp32 restatement of the reference repository, pinned to
its fixtures by tests/test_knn_oracle.py) edge for edge; no case has an undecided decision; and every case has the
property it is there for, so the GPU tests (tests/test_gpu_knn_kernels.py) exercise what they claim."""

import numpy as np
import pytest
import torch

from oracle import knn_oracle as K
from tests import edge_cases as EC
from tests import knn_cases as KC

CASES = list(KC.cases())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _crystal_counts(name, key):
    return np.concatenate([c[key] for c in KC.reference(name)["crystals"]])


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_the_oracle(name):
    nat, x, L, max_nb, _ = KC.cases()[name]
    g = KC.reference(name)
    ei, fd = K.knn_edges(nat, torch.from_numpy(np.array(x)), torch.from_numpy(np.array(L)), max_nb)
    order = torch.sort(ei[0], stable=True).indices  # grouped by source node, list order within a node
    assert ei.shape[1] == g["E"], f"{name}: {ei.shape[1]} edges in the oracle, {g['E']} in the reference"
    assert np.array_equal(ei[0][order].numpy(), g["src"]) and np.array_equal(ei[1][order].numpy(), g["dst"])
    assert np.array_equal(_bits(fd[order].numpy()), _bits(g["fd"])), f"{name}: frac_diff differs"


@pytest.mark.parametrize("name", CASES)
def test_no_undecided_decision(name):
    """A condition on the inputs, not a tolerance: every radius and cap decision is at least 1e-4 (relative) from its
    cut in float64; fp32 rounding moves d2 and the cuts by less than 1e-6."""
    g = KC.reference(name)
    print(f"{name}: E {g['E']} radius margin {g['radius_margin']:.2e} cap margin {g['cap_margin']:.2e}")
    assert g["radius_margin"] >= KC.MARGIN and g["cap_margin"] >= KC.MARGIN


@pytest.mark.parametrize("name", KC.EXACT)
def test_exact_crystals_are_exact_in_fp32(name):
    nat, x, L, _, _ = KC.cases()[name]
    off = 0
    for b, (n, c) in enumerate(zip(nat, KC.reference(name)["crystals"])):
        d32 = KC.d2_fp32(x[off:off + n], L[b])
        assert np.array_equal(d32.astype(np.float64), c["d2"]), f"{name} crystal {b}: fp32 d2 is not exact"
        off += n


@pytest.mark.parametrize("name", CASES)
def test_cases_stay_within_the_limits(name):
    nat, x, _, _, per_atom = KC.cases()[name]
    g = KC.reference(name)
    assert max(nat) <= KC.MAX_ATOMS and len(x) == sum(nat)
    assert g["deg"].max(initial=0) <= KC.MAX_DEG
    assert g["E"] <= per_atom * sum(nat)
    assert g["deg"].sum() == g["E"] and np.array_equal(np.bincount(g["dst"], minlength=sum(nat)), g["deg"])  # symmetric


def test_refusal_cases_are_outside_them():
    r = KC.refusal_cases()
    nat, x, L, max_nb, per_atom = r["above_256_edges"]
    g = KC.graph(nat, x, L, max_nb)
    assert g["deg"].min() == 304 and g["E"] <= per_atom * sum(nat)  # (the capacity is not what refuses it)
    assert min(g["radius_margin"], g["cap_margin"]) >= KC.MARGIN
    nat, x, L, max_nb, per_atom = r["above_capacity"]
    g = KC.graph(nat, x, L, max_nb)
    assert g["E"] == 72 and per_atom * sum(nat) == 4 and g["deg"].max() <= KC.MAX_DEG


def test_the_properties_the_cases_are_there_for():
    ref = KC.reference
    # self-image edges only: the earlier-cell rule and fd = -/+ cell are the whole answer
    g = ref("sc1")
    assert g["E"] == 6 and (g["src"] == 0).all() and (g["dst"] == 0).all()
    assert sorted(map(tuple, g["fd"].tolist())) == sorted(
        [tuple(float(s * (k == a)) for k in range(3)) for a in range(3) for s in (-1, 1)])
    assert g["fd"][:3].sum(1).tolist() == [1.0, 1.0, 1.0]  # the kept direction: cells (-1,0,0), (0,-1,0), (0,0,-1), fd = -cell
    # ties straddle the cap and the tie shell is kept whole
    for name, deg in (("bcc_cap6", 8), ("diamond", 28), ("sc64", 26), ("sc256", 26), ("sc64_cap12", 18), ("sc64_cap1", 6)):
        c = ref(name)["crystals"][0]
        assert c["tie_at_cap"].all() and (ref(name)["deg"] == deg).all(), name
    # candidates per atom: above 64, exactly 256, above 256
    assert (_crystal_counts("sc64", "ncand") == 256).all() and (_crystal_counts("sc256", "ncand") == 256).all()
    assert (_crystal_counts("sc64_fine", "ncand") == 304).all()
    assert _crystal_counts("n65", "ncand").min() > 64
    # index 255 in both key bytes, as atom1 and as atom2 of kept candidates, and as src and dst of edges
    for name in ("sc256", "ragged_1_between"):
        c = ref(name)["crystals"][-1]
        i, j, _ = c["directed"].T
        assert (i == 255).any() and c["kept"][:, 255].any() and c["kept"][255].any()
        off = len(ref(name)["deg"]) - 256
        assert (ref(name)["src"] == off + 255).any() and (ref(name)["dst"] == off + 255).any()
    # the cap's boundary counts
    assert (_crystal_counts("fcc_cap18", "ncand") == 18).all() and (_crystal_counts("fcc_cap17", "ncand") == 18).all()
    nc = _crystal_counts("n63_cap252", "ncand")
    cut = ref("n63_cap252")["crystals"][0]["cut"]
    assert (nc == 252).any() and (nc == 253).any()
    assert np.isinf(cut[nc == 252]).all() and np.isfinite(cut[nc == 253]).all()
    # uncapped, and a cap nobody reaches: every pair within the radius, degree 256 = the supported maximum
    for m in (0, -1, 256, 300):
        assert (ref(f"sc64_cap{m}")["deg"] == 256).all()
    # one-sided pairs, and both outcomes of the one-direction rule on them
    c = ref("cluster")["crystals"][0]
    assert c["one_sided"] > 0
    far = 13
    kept_by_far = c["kept"][far] & ~c["kept"].transpose(1, 0, 2)[:, :, ::-1][far]  # (far, j, c) kept, (j, far, -c) dropped
    js = np.nonzero(kept_by_far.any(1))[0]
    assert (js < far).any() and (js > far).any()
    e = set(zip(ref("cluster")["src"].tolist(), ref("cluster")["dst"].tolist()))
    lo = [j for j in js if j < far and not (c["kept"][far, j] & ~kept_by_far[j]).any()]
    hi = [j for j in js if j > far and not (c["kept"][far, j] & ~kept_by_far[j]).any()]
    assert lo and hi
    assert all((j, far) in e and (far, j) in e for j in lo)          # kept by the higher index: an edge both ways
    assert all((j, far) not in e and (far, j) not in e for j in hi)  # kept by the lower index only: no edge
    for name in ("random_mid", "random_256"):
        assert sum(c["one_sided"] for c in ref(name)["crystals"]) > 0
    # atoms without edges
    assert ref("edgeless1")["E"] == 0 and ref("edgeless_batch")["E"] == 0
    g = ref("mixed_edgeless")
    run = max(len(r) for r in "".join("0" if d == 0 else "1" for d in g["deg"]).split("1"))
    assert run >= 300 and g["E"] > 0 and g["deg"][0] > 0 and g["deg"][-1] > 0
    t = KC.segment_tiles(g["deg"])
    assert (0, 256) in t and g["deg"][:256].sum() > 0  # the break at 256 nodes, in a tile that has rows
    g = ref("edgeless_run600")
    t = KC.segment_tiles(g["deg"])
    assert any(b - a == 256 and g["deg"][a:b].sum() == 0 and a > 0 for a, b in t)  # a tile of 256 nodes without a row
    # one node per tile next to many nodes per tile
    d = ref("hub_and_leaves")["deg"]
    assert ((d >= 200) & (d <= 256)).sum() == 63 and (d == 1).sum() == 88 and (d == 0).sum() == 2
    assert d[5] == 1 and d[6] >= 200 and d[6 + 63] == 1
    t = KC.segment_tiles(d)
    assert sum(b - a == 1 for a, b in t) >= 62 and any(b - a > 64 for a, b in t)
    assert all(d[a:b].sum() <= 256 and b - a <= 256 for name in CASES for d in [ref(name)["deg"]]
               for a, b in KC.segment_tiles(d))
    # the same crystal alone and inside a batch: the same edges shifted by its node offset
    nat = KC.cases()["ragged_1_between"][0]
    g, alone = ref("ragged_1_between"), ref("sc256")
    off = nat[0] + nat[1]
    m = g["src"] >= off
    assert np.array_equal(g["src"][m] - off, alone["src"]) and np.array_equal(g["dst"][m] - off, alone["dst"])
    assert np.array_equal(_bits(g["fd"][m]), _bits(alone["fd"]))
    assert nat[1] == 1 and g["deg"][nat[0]] == 6
    # unwrapped coordinates in the random cases
    for name in ("random_small", "random_mid", "random_256"):
        x = KC.cases()[name][1]
        assert x.min() < 0 and x.max() > 1


def test_message_reference_equals_the_fc_one_on_fc_edges():
    """msg_ref64 / msg_base32 on an explicit edge list are edge_cases.ref64 / base32 when the list is the fc one and
    fd the wrapped difference (the definitions differ only in the graph); an edgeless node's row is exactly 0."""
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict
    w = EC.layer_weights(synthetic_state_dict(default_config()), 0)
    nat = [3, 1, 4]
    N = sum(nat)
    frac = EC.frac_coords(nat)
    PQ = EC.pq("normal", N, 2)
    ei, ej = EC.fc_edges(nat)
    fd = EC.rem1(frac[ej] - frac[ei])
    assert np.array_equal(KC.fourier_args(fd), EC.fourier_args(frac, ei, ej))
    a = KC.msg_ref64(ei, ej, fd, N, PQ, w)
    assert np.abs(a - EC.ref64(nat, frac, PQ, w)).max() <= 1e-13 * np.abs(a).max()
    b = KC.msg_base32(ei, ej, fd, N, PQ, w)
    assert np.abs(b - EC.base32(nat, frac, PQ, w)).max() <= 1e-5 * np.abs(b).max()
    keep = ei != 3  # node 3 (the one-atom crystal) without its self edge
    a0 = KC.msg_ref64(ei[keep], ej[keep], fd[keep], N, PQ, w)
    assert (a0[:, 3] == 0).all() and np.array_equal(np.delete(a0, 3, 1), np.delete(a, 3, 1))
    assert (KC.msg_base32(ei[keep], ej[keep], fd[keep], N, PQ, w)[:, 3] == 0).all()
    assert (KC.msg_ref64(ei[:0], ej[:0], fd[:0], N, PQ, w) == 0).all()
