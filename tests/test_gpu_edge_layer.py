"""One CSP layer's message path (chm_debug_edge_layer: the decoder's own per-layer edge block, on the schedule the
model's options give it) against a float64 reference, per layer and per schedule.

    agg[c][i] = mean_j SiLU(SiLU(D f_ij + P_c[i] + Q_c[j]) W2^T + b2)

Operands, reference, baseline and metric: tests/edge_cases.py (pinned to the oracle on the CPU by
tests/test_edge_cases.py). Metric per output row: e = max_k |agg - ref64| / max_k |ref64|; rows whose reference
maximum is below 1e-30 must come out below 1e-30. Gate: max e <= 16 x max(e of the float32 chain on the CPU, 2^-24).
8 is the project's factor for one split GEMM against a float32 matmul and the float32 chain already holds both
GEMMs' float32 error; the further factor 2 is for the two v_exp / v_rcp SiLUs. Every case prints e, the baseline
and their ratio (pytest -s); the table is in profiles/r8/edge_unit/README.md.

The Fourier arguments are part of the operation: split16 runs edge layer 1 on unordered pairs by default, where the
reverse edge takes the forward edge's fp32 argument negated, so those schedules are measured against the reference
with pairs=True and the directed ones (option edge_pairs 0, bf16x3, f32) against the directed reference. For the
same reason the schedules fall into two groups, directed and pairs, each bit-identical within itself.

Guards: d_agg is followed by 8 sentinel rows that must stay untouched, d_PQ by NaN rows inside its allocation, and
outputs must be finite. A HIP error from the hook ends the session: nothing else runs on the device after a fault.

Crystals of 81 to 256 atoms (EC.BIG_SHAPES, the rest of the range a fully connected batch accepts) run through the
same tests in cases of their own (test_accuracy_big, test_schedules_big, ...): the second pass of the pair grid's
flag polling (128 atoms: 65 pair tiles), lists whose pair ranges all start at pair tile 0, nodes cut by a tile edge
at every offset (255) and nodes of exactly one row tile (256). Their table: profiles/big_crystals/README.md.

Findings: see profiles/r8/edge_unit/README.md."""

import functools

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict
from tests import edge_cases as EC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
H = EC.H
L = default_config()["num_layers"]
CGUARD, PQGUARD = 8, 16
SENT = -12345.6787109375  # d_agg's pre-fill (exact in fp32)
MATHS = ["split16", "bf16x3", "f32"]
# every launch-schedule option these tests touch, at the model's defaults
DEFAULTS = dict(edge_pairs=1, edge_pairs_layer=1, edge_rows=1, edge_rows_nowait=0, edge_rows_short=1, edge_layer=1,
                edge_lag=8, edge_layer_min=256, node_ps=0)


def _decoder(sd):
    from chemeleon_amd.modules.cspnet import CSPNet
    c = default_config()
    net = CSPNet(hidden_dim=c["hidden_dim"], time_dim=c["time_dim"], text_dim=c["text_dim"], num_layers=c["num_layers"],
                 max_atoms=c["max_atoms"], act_fn=c["act_fn"], dis_emb=c["dis_emb"], num_freqs=c["num_freqs"],
                 edge_style=c["edge_style"], cutoff=c["cutoff"], max_neighbors=c["max_neighbors"], ln=c["ln"], ip=c["ip"],
                 smooth=c["smooth"], pred_atom_types=c["pred_atom_types"])
    net.load_state_dict(sd)
    return net.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _sd():
    return synthetic_state_dict(default_config())


@pytest.fixture(scope="module")
def dec():
    """A module-private decoder: its options never reach the shared fixtures of other modules."""
    d = _decoder(_sd())
    yield d
    del d
    torch.cuda.empty_cache()


def configure(dec, math="split16", **opts):
    """The math mode and every schedule option at its default, then `opts`."""
    if dec.get_math() != math:
        dec.set_math(math)
    for k, v in {**DEFAULTS, **opts}.items():
        if dec._options.get(k, DEFAULTS[k]) != v:
            dec.set_option(k, v)


@functools.lru_cache(maxsize=None)
def _weights(layer):
    return EC.layer_weights(_sd(), layer)


@functools.lru_cache(maxsize=None)
def _case(shape, family, layer, pairs_def, frac_kind="uniform"):
    """(frac, PQ [2, N, 2H], ref64 [2, N, H], the float32 chain's max e per conditioning count {1, 2}), computed once."""
    nat = EC.ALL_SHAPES[shape]
    frac = EC.frac_coords(nat, frac_kind)
    PQ = EC.pq(family, sum(nat), 2)
    w = _weights(layer)
    ref = EC.ref64(nat, frac, PQ, w, pairs_def)
    ref.setflags(write=False)
    b32 = EC.base32(nat, frac, PQ, w, pairs_def)
    base = {p: EC.max_row_error(b32[:p], ref[:p]) for p in (1, 2)}
    return frac, PQ, ref, base


def run_layer(dec, nat, pairs, layer, frac, PQ, split=False, max_pairs=None):
    """One chm_debug_edge_layer call on a private batch. Returns agg [pairs, N, H] (numpy), and with split the raw
    split rows and exponents, after checking the guards."""
    N = sum(nat)
    b = dec.hip_batch(nat, max_pairs=max_pairs or pairs, private=True)
    d_frac = torch.tensor(np.ascontiguousarray(frac, np.float32)).to(DEV)
    d_pq = torch.full((pairs * N + PQGUARD, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
    d_pq[:pairs * N] = torch.tensor(np.asarray(PQ[:pairs], np.float32)).reshape(pairs * N, 2 * H).to(DEV)
    d_agg = torch.full((pairs * N + CGUARD, H), SENT, dtype=torch.float32, device=DEV)
    d_split = d_exp = None
    if split:
        d_split = torch.full((pairs * N + CGUARD, 2 * H), 7.0, dtype=torch.float16, device=DEV)
        d_exp = torch.full((pairs * N + CGUARD,), 0x55555555, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    rc = lib.chm_debug_edge_layer(b.handle, pairs, layer, _lib.ptr(d_frac), d_frac.numel(), _lib.ptr(d_pq), pairs * N * 2 * H,
                                  _lib.ptr(d_agg), pairs * N * H, _lib.ptr(d_split), _lib.ptr(d_exp), _lib.stream_handle())
    if rc == -2:  # a HIP error (a fault included): nothing more may run on this device in this session
        pytest.exit(f"chm_debug_edge_layer: {lib.chm_last_error().decode(errors='replace')}", returncode=3)
    assert rc == 0, lib.chm_last_error()
    torch.cuda.synchronize()
    short = lib.chm_batch_short_row_tiles(b.handle)
    agg = d_agg[:pairs * N]
    assert bool(torch.isfinite(agg).all()), "non-finite outputs: a guard row reached the arithmetic"
    assert torch.equal(d_agg[pairs * N:].view(torch.int32),
                       torch.full((CGUARD, H), SENT, device=DEV).view(torch.int32)), "rows past agg were written"
    assert bool(torch.isnan(d_pq[pairs * N:]).all()), "the caller's PQ guard rows were written"
    out = agg.reshape(pairs, N, H).cpu().numpy()
    if split:
        assert bool((d_split[pairs * N:] == 7.0).all()) and bool((d_exp[pairs * N:] == 0x55555555).all()), \
            "rows past the split agg were written"
        return out, d_split[:pairs * N].cpu().numpy(), d_exp[:pairs * N].cpu().numpy(), short
    return out, short


def check_gate(tag, agg, ref, base):
    e = EC.max_row_error(agg, ref)
    print(f"{tag}: e {e:.3e} baseline {base:.3e} ratio {e / max(base, EC.U):.2f}")
    assert e <= EC.gate(base), f"{tag}: e {e:.3e} above 16 x the float32 chain's {max(base, EC.U):.3e}"
    return e


# ---------------------------------------------------------------- accuracy against float64, every math mode

@pytest.mark.parametrize("family", EC.FAMILIES)
@pytest.mark.parametrize("shape", list(EC.SHAPES))
@pytest.mark.parametrize("math", MATHS)
def test_accuracy(dec, math, shape, family):
    """The default schedule of each math mode: layers 0 and L-1, one and two conditionings."""
    configure(dec, math)
    nat = EC.SHAPES[shape]
    for layer in (0, L - 1):
        frac, PQ, ref, base = _case(shape, family, layer, math == "split16")
        for pairs in (1, 2):
            agg, _ = run_layer(dec, nat, pairs, layer, frac, PQ)
            check_gate(f"{math} {shape} {family} layer {layer} pairs {pairs}", agg, ref[:pairs], base[pairs])


@pytest.mark.parametrize("shape", ["mixed7", "17", "ragged5"])
@pytest.mark.parametrize("math", MATHS)
def test_accuracy_coincident_atoms_and_cell_edges(dec, math, shape):
    """Coordinates at 0 and at 1 - 2^-24 and coincident atoms: d = 0, d = 2^-24 and d just below 1."""
    configure(dec, math)
    nat = EC.SHAPES[shape]
    frac, PQ, ref, base = _case(shape, "normal", 0, math == "split16", "edge")
    for pairs in (1, 2):
        agg, _ = run_layer(dec, nat, pairs, 0, frac, PQ)
        check_gate(f"{math} {shape} edge coordinates pairs {pairs}", agg, ref[:pairs], base[pairs])


BIG = list(EC.BIG_SHAPES)


@pytest.mark.parametrize("shape", BIG)
def test_accuracy_big(dec, shape):
    """Crystals of 81 to 256 atoms on split16's default schedule (the pair grid from 256 row tiles, i.e. at 256 and
    ragged256; two launches below): layers 0 and L-1, one and two conditionings, under the same gate."""
    configure(dec, "split16")
    nat = EC.BIG_SHAPES[shape]
    for layer in (0, L - 1):
        frac, PQ, ref, base = _case(shape, "rowscale", layer, True)
        for pairs in (1, 2):
            agg, _ = run_layer(dec, nat, pairs, layer, frac, PQ)
            check_gate(f"split16 {shape} rowscale layer {layer} pairs {pairs}", agg, ref[:pairs], base[pairs])


@pytest.mark.parametrize("shape", ["128", "256"])
@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_accuracy_big_directed_maths(dec, math, shape):
    configure(dec, math)
    nat = EC.BIG_SHAPES[shape]
    frac, PQ, ref, base = _case(shape, "normal", 0, False)
    for pairs in (1, 2):
        agg, _ = run_layer(dec, nat, pairs, 0, frac, PQ)
        check_gate(f"{math} {shape} normal layer 0 pairs {pairs}", agg, ref[:pairs], base[pairs])


@pytest.mark.parametrize("shape", ["128", "ragged256"])
def test_accuracy_big_coincident_atoms_and_cell_edges(dec, shape):
    configure(dec, "split16")
    nat = EC.BIG_SHAPES[shape]
    frac, PQ, ref, base = _case(shape, "normal", 0, True, "edge")
    for pairs in (1, 2):
        agg, _ = run_layer(dec, nat, pairs, 0, frac, PQ)
        check_gate(f"split16 {shape} edge coordinates pairs {pairs}", agg, ref[:pairs], base[pairs])


# ---------------------------------------------------------------- schedules (split16)

# option sets of tests/test_gpu_parity.py (test_edge_row_tiles_are_bit_identical, test_edge_pairs_grid_is_bit_identical,
# test_short_row_tiles_are_bit_identical, test_edge_pairs_layer2_schedules_are_bit_identical), without their forced
# repairs and timeouts. edge_layer_min 1 engages the one-grid forms at these sizes; short: the batch must (True) or
# must not (False) take 192-row tiles; grid: launches of the one-grid kernels (CHM_K_EDGE_LAYER) the call must record.
DIRECTED = [
    ("node-aligned segment tiles", dict(edge_pairs=0, edge_rows=0, edge_layer=0), False, 0),
    ("row tiles", dict(edge_pairs=0, edge_rows=1, edge_layer=0, edge_rows_short=0), False, 0),
    ("row tiles, msgbuf path", dict(edge_pairs=0, edge_rows=1, edge_rows_nowait=1, edge_layer=0, edge_rows_short=0), False, 0),
    ("short row tiles", dict(edge_pairs=0, edge_rows=1, edge_layer=0, edge_rows_short=1), True, 0),
]
PAIRS = [
    ("pairs, two launches, row tiles", dict(edge_pairs=1, edge_pairs_layer=0, edge_rows_short=0), False, 0),
    ("pairs, node-aligned segment tiles", dict(edge_pairs=1, edge_pairs_layer=0, edge_rows=0), False, 0),
    ("pairs, row tiles, msgbuf path", dict(edge_pairs=1, edge_pairs_layer=0, edge_rows_short=0, edge_rows_nowait=1), False, 0),
    ("pairs, short row tiles (the default here)", dict(edge_pairs=1), True, 0),
    ("pairs, short row tiles, msgbuf path", dict(edge_pairs=1, edge_rows_nowait=1), True, 0),
    ("pair grid", dict(edge_pairs=1, edge_pairs_layer=1, edge_layer_min=1), False, 1),
]
NO_EVENTS = ("layer_wait_timeouts", "layer_repairs", "tail_wait_timeouts", "tail_repairs", "layer_incomplete")


def grid_launches(opts, nat):
    """One-grid launches a call records under `opts` (decoder.hip edge_plan): the pair grid runs when edge layer 1
    is on pairs, the one-grid form and row tiles are on and the batch has edge_layer_min row tiles."""
    o = {**DEFAULTS, **opts}
    R = (sum(n * n for n in nat) + 255) // 256
    return int(bool(o["edge_pairs"] and o["edge_pairs_layer"] and o["edge_rows"] and o["edge_layer"]
                    and R >= o["edge_layer_min"]))


def short_tiles_of(nat, pairs, opts):
    """The mixed tiling batch creation must choose under `opts` (batch.hip short_row_tiles, through the CPU hook
    tests/test_row_tiles.py checks): -1 unless the options take 192-row tiles at all."""
    o = {**DEFAULTS, **opts}
    if not (o["edge_rows"] and o["edge_rows_short"]):
        return -1
    import ctypes
    arr = (ctypes.c_int32 * len(nat))(*nat)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return _lib.load().chm_debug_short_row_tiles(arr, len(nat), pairs, ncu, o["edge_layer_min"])


@pytest.mark.parametrize("pairs", [1, 2])
@pytest.mark.parametrize("shape", list(EC.SHAPES))
@pytest.mark.parametrize("group", ["directed", "pairs"])
def test_schedules(dec, group, shape, pairs):
    """Every schedule's agg passes the float64 gate and equals the group's first bit for bit; the device counters
    show no timeout and no repair; the schedule that was asked for is the one that ran."""
    check_schedules(dec, group, shape, pairs)


@pytest.mark.parametrize("pairs", [1, 2])
@pytest.mark.parametrize("shape", ["128", "193+", "256", "ragged256"])
@pytest.mark.parametrize("group", ["directed", "pairs"])
def test_schedules_big(dec, group, shape, pairs):
    """The same on crystals above 80 atoms. From 256 row tiles (256, ragged256) the pair grid is the default, so it
    runs under every option set that leaves it on, not only under the one that lowers edge_layer_min; the launch
    count asserted follows that rule (grid_launches). A batch with a crystal above 192 atoms (193+, 256, ragged256)
    never takes 192-row tiles; 128 takes what batch creation's rule gives an option set that asks for them: with
    one conditioning 86 short tiles (172 jobs) fit one round of the CUs, with two (344 jobs) they do not, and its
    64 uniform tiles then fill that round exactly."""
    check_schedules(dec, group, shape, pairs)


def check_schedules(dec, group, shape, pairs):
    nat = EC.ALL_SHAPES[shape]
    big = shape in EC.BIG_SHAPES
    layer = L - 1
    frac, PQ, ref, base = _case(shape, "rowscale", layer, group == "pairs")
    lib = _lib.load()
    first = None
    _lib.check(lib.chm_prof_enable(1), "chm_prof_enable")
    try:
        for name, opts, want_short, want_grid in (DIRECTED if group == "directed" else PAIRS):
            configure(dec, "split16", **opts)
            _lib.prof_events(reset=True)
            _lib.check(lib.chm_prof_reset(), "chm_prof_reset")
            agg, short = run_layer(dec, nat, pairs, layer, frac, PQ)
            ev = _lib.prof_events()
            n_grid = _lib.prof_read(_lib.K_EDGE_LAYER)[0]
            tag = f"{name} | {shape} pairs {pairs}"
            assert all(ev[k] == 0 for k in NO_EVENTS), (tag, ev)
            if not big:
                assert (short >= 0) == want_short, f"{tag}: chm_batch_short_row_tiles {short}"
                assert grid_launches(opts, nat) == want_grid
            elif max(nat) > 192:
                assert short < 0, f"{tag}: chm_batch_short_row_tiles {short} with a crystal above 192 atoms"
            else:
                assert short == (short_tiles_of(nat, pairs, opts) if want_short else -1), \
                    f"{tag}: chm_batch_short_row_tiles {short}"
                if pairs == 1:  # (the option's own wish holds where one round takes the short tiles)
                    assert (short >= 0) == want_short, f"{tag}: chm_batch_short_row_tiles {short}"
            want_grid = grid_launches(opts, nat)
            assert n_grid == want_grid, f"{tag}: {n_grid} one-grid launches"
            if want_grid:
                assert ev["layer_other_xcd"] == 0, (tag, ev)
            check_gate(tag, agg, ref[:pairs], base[pairs])
            if first is None:
                first = agg
            else:
                assert np.array_equal(first.view(np.int32), agg.view(np.int32)), f"{tag}: differs from the group's first"
    finally:
        lib.chm_prof_enable(0)
        lib.chm_prof_reset()


# ---------------------------------------------------------------- exactness

@pytest.mark.parametrize("math", MATHS)
def test_mean_of_equal_messages(math):
    """W2 = 0 and b2 = c: every message is v = SiLU(c), so a node's mean is the fp32 sequential sum of n copies of v
    divided by n. Against that loop on the CPU with v = the float32 SiLU(c), within 2 float32 ulps (the SiLU's);
    and exactly the loop over the device's own v, which the 1-atom crystal returns."""
    c, layer = 0.8125, 1
    sd = {k: v.clone() for k, v in _sd().items()}
    sd[f"csp_layer_{layer}.edge_mlp.2.weight"].zero_()
    sd[f"csp_layer_{layer}.edge_mlp.2.bias"].fill_(c)
    d = _decoder(sd)
    configure(d, math)
    nat = [1, 3, 16, 17, 80]
    N = sum(nat)
    agg, _ = run_layer(d, nat, 2, layer, EC.frac_coords(nat), EC.pq("normal", N, 2))
    del d
    torch.cuda.empty_cache()

    def seq_mean(v, n):
        s = np.float32(0.0)
        for _ in range(n):
            s = np.float32(s + v)
        return np.float32(s / np.float32(n))

    v_cpu = np.float32(torch.nn.functional.silu(torch.tensor(c, dtype=torch.float32)).item())
    v_dev = agg[0, 0, 0]
    n_of = EC.node_counts(nat)
    for i in range(N):
        n = int(n_of[i])
        want, want_dev = seq_mean(v_cpu, n), seq_mean(v_dev, n)
        ulp = np.spacing(np.abs(want))
        err = np.abs(agg[:, i].astype(np.float64) - np.float64(want)).max()
        if i in (0, 1, 4, 20, 37):
            print(f"{math} n={n}: agg {agg[0, i, 0]!r} cpu loop {want!r} ({err / ulp:.1f} ulp), device-v loop {want_dev!r}")
        assert err <= 2 * ulp, f"n = {n}: {agg[0, i, 0]!r} against {want!r}"
        assert (agg[:, i] == want_dev).all(), f"n = {n}: not the sequential sum of n copies of {v_dev!r} over n"


@pytest.mark.parametrize("opts", [dict(), dict(edge_pairs=0, edge_rows_short=0),
                                  dict(edge_pairs=1, edge_pairs_layer=1, edge_layer_min=1)],
                         ids=["default", "directed", "pair-grid"])
def test_rows_do_not_depend_on_their_neighbours(dec, opts):
    """Two crystals swapped in natoms, their coordinates and PQ rows moved along: agg's rows move bit for bit, though
    the tiles cut the batch elsewhere."""
    check_swapped_crystals(dec, opts, EC.SHAPES["ragged5"])  # [23, 7, 40, 1, 80]


@pytest.mark.parametrize("opts", [dict(), dict(edge_pairs=1, edge_pairs_layer=1, edge_layer_min=1)],
                         ids=["default", "pair-grid"])
def test_rows_do_not_depend_on_their_neighbours_big(dec, opts):
    """The same with crystals of 130 and 200 atoms (223 row tiles): the 200-atom crystal's nodes, each most of a row
    tile, meet the tile edges at other offsets once the 7-atom and 1-atom crystals change places."""
    check_swapped_crystals(dec, opts, [130, 7, 200, 1])


def check_swapped_crystals(dec, opts, nat):
    configure(dec, "split16", **opts)
    N = sum(nat)
    off = np.concatenate([[0], np.cumsum(nat)])
    order = list(range(len(nat)))
    order[1], order[3] = 3, 1  # crystals 1 and 3 swapped
    perm = np.concatenate([np.arange(off[g], off[g + 1]) for g in order])
    frac, PQ = EC.frac_coords(nat), EC.pq("rowscale", N, 2)
    a0, _ = run_layer(dec, nat, 2, 0, frac, PQ)
    a1, _ = run_layer(dec, [nat[g] for g in order], 2, 0, frac[perm], PQ[:, perm])
    assert np.array_equal(a0[:, perm].view(np.int32), a1.view(np.int32))


# ---------------------------------------------------------------- split agg rows (pre-split node GEMMs)

@pytest.mark.parametrize("shape,family", [(s, f) for s in ["mixed7", "ragged5", "1"] for f in ["rowscale", "chunkdead"]]
                         + [("256", "rowscale")])
def test_split_agg_rows(dec, shape, family):
    """Option node_ps: the layer writes agg as split rows + packed chunk exponents. Per 128-column chunk
    |(hi + lo) 2^e - agg_fp32| <= 2^-22 max|chunk|: the scaled value is below 1, hi is off by at most 2^-12, lo keeps
    11 more bits or bottoms out at 2^-25, in all 2^-23 2^e, and 2^e <= 2 max. e is the frexp exponent of the chunk's
    maximum (store_split_row512's layout); a dead chunk has exponent 0 and all-zero halves."""
    configure(dec, "split16", node_ps=1)
    nat = EC.ALL_SHAPES[shape]
    N = sum(nat)
    frac, PQ = EC.frac_coords(nat), EC.pq(family, N, 2)
    w = _weights(0)
    if family == "chunkdead":  # agg chunk 2 exactly 0: W2 rows and b2 of its columns zero on a private model
        sd = {k: v.clone() for k, v in _sd().items()}
        sd["csp_layer_0.edge_mlp.2.weight"][256:384] = 0
        sd["csp_layer_0.edge_mlp.2.bias"][256:384] = 0
        d = _decoder(sd)
        configure(d, "split16", node_ps=1)
    else:
        d = dec
    agg, split, exps, _ = run_layer(d, nat, 2, 0, frac, PQ, split=True)
    val, hi, lo, e = EC.split_rows_value(split, exps)
    a = agg.reshape(2 * N, H).astype(np.float64)
    worst = 0.0
    for c in range(4):
        s = slice(128 * c, 128 * c + 128)
        m = np.abs(a[:, s]).max(1)
        dead = m == 0
        assert (np.abs(val[:, s] - a[:, s]).max(1) <= 2.0 ** -22 * m).all(), f"chunk {c}"
        assert np.array_equal(e[:, c], np.where(dead, 0, np.frexp(m)[1])), f"chunk {c}: exponents"
        assert (hi[dead][:, s] == 0).all() and (lo[dead][:, s] == 0).all()
        worst = max(worst, float((np.abs(val[:, s] - a[:, s]).max(1) / np.where(dead, 1, m)).max()))
        if family == "chunkdead" and c == 2:
            assert dead.all()
    print(f"split agg {shape} {family}: worst chunk error {worst / 2.0 ** -22:.3f} x 2^-22 max|chunk|")
    if d is not dec:
        del d
        torch.cuda.empty_cache()
    else:  # the fp32 agg of the pre-split batch is the block's own fp32 form
        configure(dec, "split16")
        agg0, _ = run_layer(dec, nat, 2, 0, frac, PQ)
        assert np.array_equal(agg0.view(np.int32), agg.view(np.int32))


# ---------------------------------------------------------------- refusals on a real batch

def test_hook_refuses_what_the_batch_cannot_take(dec):
    configure(dec, "split16")
    nat = [3, 5]
    N = 8
    b = dec.hip_batch(nat, max_pairs=1, private=True)
    lib = _lib.load()
    x = torch.zeros(4 * N * 2 * H, device=DEV)
    p = _lib.ptr(x)

    def call(pairs=1, layer=0, n_frac=3 * N, split=None, exp=None):
        n = n_frac // 3
        return lib.chm_debug_edge_layer(b.handle, pairs, layer, p, n_frac, p, pairs * n * 2 * H, p, pairs * n * H, split, exp,
                                        _lib.stream_handle())
    assert call(pairs=2) == -1 and b"pairs" in lib.chm_last_error()
    assert call(layer=L) == -1 and b"layer" in lib.chm_last_error()
    assert call(n_frac=3 * N + 3) == -1 and b"n_frac" in lib.chm_last_error()
    assert call(split=p, exp=p) == -3 and b"d_agg_split" in lib.chm_last_error()
    from chemeleon_amd.modules.cspnet import HipBatch
    k = HipBatch(dec.hip_model(), nat, 1, knn=True)  # a knn batch of the same model
    rc = lib.chm_debug_edge_layer(k.handle, 1, 0, p, 3 * N, p, N * 2 * H, p, N * H, None, None, _lib.stream_handle())
    assert rc == -3 and b"knn" in lib.chm_last_error()
    torch.cuda.synchronize()
