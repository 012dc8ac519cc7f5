"""The radius-graph ("knn") edge path alone: the graph kernels (k_knn_pairs, k_knn_select, k_knn_place and the host
part of knn_build, through chm_knn_edges) against an exact reference, and one CSP layer's message path on knn graphs
(chm_debug_knn_edge_layer: knn_build, edge_features and edge_block as a decoder call runs them, on the node-aligned
segment tiles only knn batches take) against float64.

Cases and references: tests/knn_cases.py, held against the oracle and checked for their properties on the CPU by
tests/test_knn_cases.py. No case has a radius or cap decision within 1e-4 (relative) of its cut, fp32 moves them by
less than 1e-6, so graphs are compared exactly: edge count, src, dst, bit-identical frac_diff, out-degrees. The
caller's buffers carry guard elements past `capacity`; every build is run twice, each time after a build on other
coordinates, and must give identical bytes (stale scratch would show).

Message path: agg[c][i] = mean over i's edges of SiLU(SiLU(D f(fd) + P_c[i] + Q_c[j]) W2^T + b2) on the reference's
edge list with fd as given, count = max(deg, 1). Metric and gate are those of tests/test_gpu_edge_layer.py: per row
e = max_k |agg - ref64| / max_k |ref64|, max e <= 16 x max(e of the float32 chain on the CPU, 2^-24); rows of
edgeless nodes must be exactly 0.0. Every case prints e, the baseline and their ratio (pytest -s); the table is in
profiles/r16/knn_unit/README.md.

Refusals (each decided on the host before anything is placed, as read in knn_build: k_knn_pairs / k_knn_select write
only scratch sized by the candidates, n^2 27 per crystal, and k_knn_place runs after both checks): a node above 256
edges, a graph above the batch's capacity, a caller capacity below E (nothing copied), a crystal of 257 atoms.

A HIP error from either entry point ends the session: nothing else runs on the device after a fault.

Segment tiles reached (knn_cases.segment_tiles restates the host's cut): one node per tile (degrees 248-256), up to
256 nodes per tile, the break at 256 nodes (mixed_edgeless) and a tile of 256 nodes without a single row
(edgeless_run600; its row exponents are read at row0 - 1 >= 0 and unused).

Findings: see profiles/r16/knn_unit/README.md."""

import functools

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict
from tests import edge_cases as EC
from tests import knn_cases as KC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
H = EC.H
L = default_config()["num_layers"]
GUARD, CGUARD, PQGUARD = 16, 8, 16
SENT = -12345.6787109375  # exact in fp32
ISENT = -7
UNSUPPORTED = -3


@functools.lru_cache(maxsize=None)
def _sd():
    return synthetic_state_dict(default_config())


@pytest.fixture(scope="module")
def dec():
    """A module-private decoder in split16 (knn batches need it): its options never reach other modules."""
    from chemeleon_amd.modules.cspnet import CSPNet
    c = default_config()
    d = CSPNet(hidden_dim=c["hidden_dim"], time_dim=c["time_dim"], text_dim=c["text_dim"], num_layers=c["num_layers"],
               max_atoms=c["max_atoms"], act_fn=c["act_fn"], dis_emb=c["dis_emb"], num_freqs=c["num_freqs"],
               edge_style="knn", cutoff=c["cutoff"], max_neighbors=c["max_neighbors"], ln=c["ln"], ip=c["ip"],
               smooth=c["smooth"], pred_atom_types=c["pred_atom_types"])
    d.load_state_dict(_sd())
    d = d.to(DEV).eval()
    if d.get_math() != "split16":
        d.set_math("split16")
    yield d
    del d
    torch.cuda.empty_cache()


def _batch(dec, nat, max_nb, per_atom, pairs=1):
    from chemeleon_amd.modules.cspnet import HipBatch
    return HipBatch(dec.hip_model(), nat, pairs, knn=True, max_neighbors=max_nb, knn_edges_per_atom=per_atom)


def _fatal(rc, what):
    if rc == -2:  # a HIP error (a fault included): nothing more may run on this device in this session
        pytest.exit(f"{what}: {_lib.load().chm_last_error().decode(errors='replace')}", returncode=3)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32)).to(DEV)


def knn_edges(b, x, lat, capacity):
    """One chm_knn_edges call into guarded buffers. Returns (rc, E, src, dst, fd) with the whole buffers (capacity +
    GUARD elements) as numpy arrays."""
    src = torch.full((capacity + GUARD,), ISENT, dtype=torch.int32, device=DEV)
    dst = torch.full((capacity + GUARD,), ISENT, dtype=torch.int32, device=DEV)
    fd = torch.full((capacity + GUARD, 3), SENT, dtype=torch.float32, device=DEV)
    n = _lib.c_i64(-1)
    rc = _lib.load().chm_knn_edges(b.handle, _lib.ptr(x), _lib.ptr(lat), _lib.ptr(src), _lib.ptr(dst), _lib.ptr(fd),
                                   capacity, _lib.ctypes.byref(n), _lib.stream_handle())
    _fatal(rc, "chm_knn_edges")
    torch.cuda.synchronize()
    return rc, n.value, src.cpu().numpy(), dst.cpu().numpy(), fd.cpu().numpy()


def _untouched(src, dst, fd, start):
    return bool((src[start:] == ISENT).all() and (dst[start:] == ISENT).all() and
                np.array_equal(fd[start:].view(np.int32), np.full_like(fd[start:], SENT).view(np.int32)))


def _other(x):
    """Other coordinates for the build in between: the atoms in reverse order, scaled and shifted."""
    return (np.asarray(x, np.float32) * np.float32(0.97) + np.float32(0.011))[::-1].copy()


# ---------------------------------------------------------------- the graph kernels

@pytest.mark.parametrize("name", list(KC.cases()))
def test_graph_equals_the_reference(dec, name):
    nat, x, lat, max_nb, per_atom = KC.cases()[name]
    g = KC.reference(name)
    E, N = g["E"], sum(nat)
    b = _batch(dec, nat, max_nb, per_atom)
    dx, dl, dother = _dev(x), _dev(lat), _dev(_other(x))
    cap = E + 7
    outs = []
    for _ in range(2):
        rc, _, _, _, _ = knn_edges(b, dother, dl, cap)  # (may be refused: other coordinates, other graph)
        assert rc in (0, UNSUPPORTED), _lib.load().chm_last_error()
        rc, n, src, dst, fd = knn_edges(b, dx, dl, cap)
        assert rc == 0, _lib.load().chm_last_error()
        assert n == E, f"{name}: {n} edges on the device, {E} in the reference"
        assert _untouched(src, dst, fd, E), f"{name}: elements past the edge count were written"
        outs.append((src, dst, fd))
    assert all(np.array_equal(a, c) for a, c in zip(outs[0][:2], outs[1][:2])), f"{name}: two builds differ"
    assert np.array_equal(outs[0][2].view(np.int32), outs[1][2].view(np.int32)), f"{name}: two builds differ in frac_diff"
    src, dst, fd = (a[:E] for a in outs[0])
    assert np.array_equal(np.bincount(src, minlength=N) if E else np.zeros(N, np.int64), g["deg"]), f"{name}: out-degrees"
    assert np.array_equal(src, g["src"]) and np.array_equal(dst, g["dst"]), f"{name}: edge lists differ"
    assert np.array_equal(fd.view(np.int32), g["fd"].view(np.int32)), f"{name}: frac_diff differs"
    print(f"{name}: N {N} E {E} degrees {g['deg'].min()}..{g['deg'].max()} exact")


def test_a_node_above_256_edges_is_refused_and_the_batch_stays_usable(dec):
    nat, x, lat, max_nb, per_atom = KC.refusal_cases()["above_256_edges"]
    b = _batch(dec, nat, max_nb, per_atom)
    cap = per_atom * sum(nat)
    rc, _, src, dst, fd = knn_edges(b, _dev(x), _dev(lat), cap)
    assert rc == UNSUPPORTED and b"more than 256 edges" in _lib.load().chm_last_error()
    assert _untouched(src, dst, fd, 0)
    # the same batch (uncapped, 64 atoms) then builds the a = 4 supercell: degree 256 exactly, the supported maximum
    nat2, x2, lat2, _, _ = KC.cases()["sc64_cap0"]
    assert nat2 == nat
    g = KC.reference("sc64_cap0")
    rc, n, src, dst, fd = knn_edges(b, _dev(x2), _dev(lat2), cap)
    assert rc == 0 and n == g["E"] == 64 * 256
    assert np.array_equal(src[:n], g["src"]) and np.array_equal(dst[:n], g["dst"])
    assert np.array_equal(fd[:n].view(np.int32), g["fd"].view(np.int32)) and _untouched(src, dst, fd, n)


def test_a_graph_above_the_batch_capacity_is_refused(dec):
    nat, x, lat, max_nb, per_atom = KC.refusal_cases()["above_capacity"]
    b = _batch(dec, nat, max_nb, per_atom)
    rc, _, src, dst, fd = knn_edges(b, _dev(x), _dev(lat), 128)
    err = _lib.load().chm_last_error()
    assert rc == UNSUPPORTED and b"72 edges" in err and b"capacity 4" in err and b"knn_edges_per_atom" in err
    assert _untouched(src, dst, fd, 0)


def test_a_caller_capacity_below_the_edge_count_copies_nothing(dec):
    nat, x, lat, max_nb, per_atom = KC.cases()["fcc"]
    E = KC.reference("fcc")["E"]
    b = _batch(dec, nat, max_nb, per_atom)
    for cap in (E - 1, 0):
        rc, n, src, dst, fd = knn_edges(b, _dev(x), _dev(lat), cap)
        assert rc == 0 and n == E
        assert _untouched(src, dst, fd, 0)
    rc, n, src, dst, fd = knn_edges(b, _dev(x), _dev(lat), E)  # exactly E: copied
    assert rc == 0 and n == E and np.array_equal(src[:E], KC.reference("fcc")["src"]) and _untouched(src, dst, fd, E)


def test_a_crystal_of_257_atoms_is_refused_at_batch_creation(dec):
    with pytest.raises(Exception, match="256 atoms"):
        _batch(dec, [4, 257], 20, KC.PER_ATOM)
    _batch(dec, [4, 256], 20, KC.PER_ATOM)


# ---------------------------------------------------------------- the message path on knn graphs

MSG_CASES = ["bcc_cap6", "sc64", "ragged_small", "mixed_edgeless", "edgeless_run600", "edgeless_batch", "hub_and_leaves"]


@functools.lru_cache(maxsize=None)
def _weights(layer):
    return EC.layer_weights(_sd(), layer)


@functools.lru_cache(maxsize=None)
def _msg_case(name, family, layer):
    """(PQ [2, N, 2H], ref64 [2, N, H], the float32 chain's max e per conditioning count {1, 2}), computed once."""
    g = KC.reference(name)
    N = len(g["deg"])
    PQ = EC.pq(family, N, 2)
    w = _weights(layer)
    ref = KC.msg_ref64(g["src"], g["dst"], g["fd"], N, PQ, w)
    ref.setflags(write=False)
    b32 = KC.msg_base32(g["src"], g["dst"], g["fd"], N, PQ, w)
    return PQ, ref, {p: EC.max_row_error(b32[:p], ref[:p]) for p in (1, 2)}


def run_knn_layer(dec, case, pairs, layer, PQ):
    """One chm_debug_knn_edge_layer call on a private knn batch of `case` = (natoms, frac, lattices, max_nb,
    per_atom). Returns agg [pairs, N, H] (numpy) after checking the guards."""
    nat, x, lat, max_nb, per_atom = case
    N = sum(nat)
    b = _batch(dec, nat, max_nb, per_atom, pairs)
    d_frac, d_lat = _dev(x), _dev(lat)
    d_pq = torch.full((pairs * N + PQGUARD, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
    d_pq[:pairs * N] = torch.tensor(np.asarray(PQ[:pairs], np.float32)).reshape(pairs * N, 2 * H).to(DEV)
    d_agg = torch.full((pairs * N + CGUARD, H), SENT, dtype=torch.float32, device=DEV)
    lib = _lib.load()
    rc = lib.chm_debug_knn_edge_layer(b.handle, pairs, layer, _lib.ptr(d_frac), d_frac.numel(), _lib.ptr(d_lat),
                                      d_lat.numel(), _lib.ptr(d_pq), pairs * N * 2 * H, _lib.ptr(d_agg), pairs * N * H,
                                      _lib.stream_handle())
    _fatal(rc, "chm_debug_knn_edge_layer")
    assert rc == 0, lib.chm_last_error()
    torch.cuda.synchronize()
    agg = d_agg[:pairs * N]
    assert bool(torch.isfinite(agg).all()), "non-finite outputs: a guard row reached the arithmetic"
    assert torch.equal(d_agg[pairs * N:].view(torch.int32),
                       torch.full((CGUARD, H), SENT, device=DEV).view(torch.int32)), "rows past agg were written"
    assert bool(torch.isnan(d_pq[pairs * N:]).all()), "the caller's PQ guard rows were written"
    return agg.reshape(pairs, N, H).cpu().numpy()


@pytest.mark.parametrize("family", EC.FAMILIES)
@pytest.mark.parametrize("name", MSG_CASES)
def test_message_path_accuracy(dec, name, family):
    """Layers 0 and L-1, one and two conditionings: every row within the gate, rows of edgeless nodes exactly 0.0."""
    case = KC.cases()[name]
    deg = KC.reference(name)["deg"]
    for layer in (0, L - 1):
        PQ, ref, base = _msg_case(name, family, layer)
        for pairs in (1, 2):
            agg = run_knn_layer(dec, case, pairs, layer, PQ)
            tag = f"knn {name} {family} layer {layer} pairs {pairs}"
            assert (agg[:, deg == 0].view(np.int32) == 0).all(), f"{tag}: an edgeless node's row is not exactly 0.0"
            e = EC.max_row_error(agg, ref[:pairs])
            b = base[pairs]
            print(f"{tag}: e {e:.3e} baseline {b:.3e} ratio {e / max(b, EC.U):.2f}")
            assert e <= EC.gate(b), f"{tag}: e {e:.3e} above 16 x the float32 chain's {max(b, EC.U):.3e}"


def test_rows_of_a_crystal_do_not_depend_on_the_batch(dec):
    """A crystal alone and inside a ragged batch (other tiles, other node offsets): its rows bit for bit, each node
    being one sequential sum over its own edges. For the 64-atom supercell, the one-atom crystal and an edgeless one."""
    nat, x, lat, max_nb, per_atom = KC.cases()["ragged_small"]
    N = sum(nat)
    PQ = EC.pq("rowscale", N, 2)
    whole = run_knn_layer(dec, (nat, x, lat, max_nb, per_atom), 2, 0, PQ)
    off = np.concatenate([[0], np.cumsum(nat)])
    for g in (3, 5, 2):  # SC64, SC1, BCC
        s = slice(off[g], off[g + 1])
        alone = run_knn_layer(dec, ([nat[g]], x[s], lat[g:g + 1], max_nb, per_atom), 2, 0, PQ[:, s])
        assert np.array_equal(alone.view(np.int32), whole[:, s].view(np.int32)), f"crystal {g} differs inside the batch"
    # an edgeless crystal between other neighbours: exactly 0 whatever surrounds it
    enat, ex, elat, _, _ = KC.cases()["mixed_edgeless"]
    eoff = np.concatenate([[0], np.cumsum(enat)])
    order = [4, 1, 0, 2]  # an edgeless one, then one between fcc and bcc swapped round
    sub = ([enat[g] for g in order], np.concatenate([ex[eoff[g]:eoff[g + 1]] for g in order]), elat[order], 20, KC.PER_ATOM)
    PQs = EC.pq("large", sum(sub[0]), 2)
    a = run_knn_layer(dec, sub, 2, L - 1, PQs)
    assert (a[:, [0, 1]].view(np.int32) == 0).all() and (np.abs(a[:, 2:]).max(-1) > 0).all()


def test_hook_refusals(dec):
    nat = [3, 5]
    N = 8
    lib = _lib.load()
    x = torch.zeros(4 * N * 2 * H, device=DEV)
    p = _lib.ptr(x)
    b = _batch(dec, nat, 20, KC.PER_ATOM, 1)

    def call(h=None, pairs=1, layer=0, n_frac=3 * N, n_lat=18, n_pq=None, n_agg=None, frac=p, lat=p, pq=p, agg=p):
        n = n_frac // 3
        return lib.chm_debug_knn_edge_layer(b.handle if h is None else h, pairs, layer, frac, n_frac, lat, n_lat, pq,
                                            pairs * n * 2 * H if n_pq is None else n_pq, agg,
                                            pairs * n * H if n_agg is None else n_agg, _lib.stream_handle())
    for kw, field in ((dict(frac=None), b"d_frac"), (dict(lat=None), b"d_lat"), (dict(pq=None), b"d_PQ"),
                      (dict(agg=None), b"d_agg"), (dict(pairs=0), b"pairs"), (dict(pairs=2), b"pairs"),
                      (dict(layer=-1), b"layer"), (dict(layer=L), b"layer"), (dict(n_frac=3 * N + 1), b"n_frac"),
                      (dict(n_frac=3 * N + 3), b"n_frac"), (dict(n_lat=17), b"n_lat"), (dict(n_lat=27), b"n_lat"),
                      (dict(n_pq=N * 2 * H - 1), b"n_pq"), (dict(n_agg=N * H + 1), b"n_agg"),
                      (dict(frac=_lib.ptr(x[1:])), b"aligned")):
        assert call(**kw) == -1 and field in lib.chm_last_error(), (kw, lib.chm_last_error())
    assert lib.chm_debug_knn_edge_layer(None, 1, 0, p, 3, p, 9, p, 2 * H, p, H, None) == -1
    assert b"batch" in lib.chm_last_error()
    from chemeleon_amd.modules.cspnet import HipBatch
    fc = HipBatch(dec.hip_model(), nat, 1)  # an fc batch of the same model
    assert call(h=fc.handle) == UNSUPPORTED and b"fc batch" in lib.chm_last_error()
    torch.cuda.synchronize()
