"""Parity of the HIP path (through the C ABI) with the CPU oracle and with the
reference-generated golden fixtures. Run on an MI355X: pytest -m gpu.

Tolerances (north star: 1e-4 relative fp32, atom types bit-exact):
* decoder outputs: |gpu - ref| <= 1e-4 * max(|ref|, 1) elementwise-scaled
  (rtol 1e-4 with an absolute floor of 1e-4 times the tensor's RMS scale);
* atom types: bit-exact;
* fractional coordinates: periodic distance min(|d|, 1 - |d|) <= 1e-4;
* lattices: rtol 1e-4 (absolute floor 1e-4 x max |lattice|).
"""

import ctypes
import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd.config import default_config
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds, weights_crc
from oracle import chemeleon_oracle as O

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"


def scaled_err(gpu, ref):
    gpu = np.asarray(gpu, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = max(np.sqrt(np.mean(ref ** 2)), 1e-12)
    return np.abs(gpu - ref) / np.maximum(np.abs(ref), scale)


def close(gpu, ref, rtol=1e-4, what=""):
    err = scaled_err(gpu, ref)
    assert np.isfinite(np.asarray(gpu, dtype=np.float64)).all(), f"{what}: non-finite output"
    assert err.max() <= rtol, f"{what}: max scaled error {err.max():.3e} > {rtol}"
    return err.max()


def periodic_close(gpu, ref, tol=1e-4, what=""):
    d = np.abs(np.asarray(gpu, np.float64) - np.asarray(ref, np.float64))
    d = np.minimum(d, 1.0 - d)
    assert d.max() <= tol, f"{what}: max periodic error {d.max():.3e}"
    return d.max()


def _model(T):
    from chemeleon_amd import Chemeleon
    cfg = default_config()
    cfg["timesteps"] = T
    torch.manual_seed(0)  # sigmas_norm Monte-Carlo draws, as when the fixtures were made
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def model1000():
    return _model(1000)


@pytest.fixture(scope="module")
def model100():
    return _model(100)


@pytest.fixture(scope="module")
def cn():
    c, n = synthetic_text_embeds(512)
    return c, n


# --------------------------------------------------------------------------- kernels
@pytest.fixture(autouse=True)
def _default_math(request):
    """Every test starts and ends in the default arithmetic (split16); tests that compare
    modes set them explicitly."""
    models = [request.getfixturevalue(n) for n in ("model100", "model1000") if n in request.fixturenames]
    for m in models:
        m.decoder.set_math("split16")
    yield
    for m in models:
        m.decoder.set_math("split16")


def test_fourier_features(model1000, golden):
    g = golden("decoder_ragged.npz")
    nat = g["natoms"].tolist()
    x = torch.from_numpy(g["frac"])
    b = model1000.decoder.hip_batch(nat, 1)
    feat = torch.empty(b.num_edges, 768, device=DEV)
    xd = x.to(DEV)
    _lib.check(_lib.load().chm_edge_features(b.handle, _lib.ptr(xd), _lib.ptr(feat), _lib.stream_handle()), "fe")
    e = O.fc_edges(nat)
    ref = O.fourier((x[e[1]] - x[e[0]]) % 1.0, 128)
    np.testing.assert_allclose(feat.cpu().numpy(), ref.numpy(), atol=2e-6, rtol=0)


def test_fourier_features_split(model1000, golden):
    """The sampler's split16 Fourier kernel (k_fourier_h): hi + lo reproduces the oracle features
    (cspnet.py:38-52) to fp32 rounding, hi is the fp16 rounding of the feature, and the lo part
    carries the rest (|lo| <= ulp_fp16(hi) / 2)."""
    g = golden("decoder_ragged.npz")
    nat = g["natoms"].tolist()
    x = torch.from_numpy(g["frac"])
    b = model1000.decoder.hip_batch(nat, 1)
    E = b.num_edges
    raw = torch.empty(E, 768 * 2, dtype=torch.float16, device=DEV)
    xd = x.to(DEV)
    _lib.check(_lib.load().chm_edge_features_split(b.handle, _lib.ptr(xd), _lib.ptr(raw), _lib.stream_handle()), "fs")
    r = raw.view(E, 24, 2, 32).cpu()
    hi, lo = r[:, :, 0, :].reshape(E, 768), r[:, :, 1, :].reshape(E, 768)
    e = O.fc_edges(nat)
    ref = O.fourier((x[e[1]] - x[e[0]]) % 1.0, 128)
    np.testing.assert_allclose((hi.float() + lo.float()).numpy(), ref.numpy(), atol=2e-6, rtol=0)
    # hi is the fp16 rounding of the kernel's own fp32 feature, so it can differ from fp16(ref) only
    # where ref sits within fp32 rounding of an fp16 rounding boundary
    assert (hi != ref.half()).float().mean().item() < 1e-3
    assert (lo.float().abs() <= hi.float().abs() * 2.0 ** -11 + 2.0 ** -25).all()


def test_segment_mean_matches_oracle(model1000):
    nat = [3, 7, 1, 12, 40]
    b = model1000.decoder.hip_batch(nat, 2)
    gen = torch.Generator().manual_seed(3)
    msg = torch.randn(2, b.num_edges, 512, generator=gen)
    agg = torch.empty(2, b.num_nodes, 512, device=DEV)
    md = msg.to(DEV)
    _lib.check(_lib.load().chm_segment_mean(b.handle, 2, _lib.ptr(md), md.numel(), _lib.ptr(agg), agg.numel(), _lib.stream_handle()), "sm")
    e = O.fc_edges(nat)
    for c in range(2):
        ref = O.scatter_mean(msg[c], e[0], b.num_nodes)
        np.testing.assert_allclose(agg[c].cpu().numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)


def test_d3pm_bit_exact(model100, golden):
    g = golden("units.npz")
    dp = model100.d3pm
    out = dp.p_logits(torch.from_numpy(g["d3pm_logits"]).to(DEV), torch.from_numpy(g["d3pm_xt"]).to(DEV),
                      torch.from_numpy(g["d3pm_t"]).to(DEV), torch.from_numpy(g["d3pm_u"]).to(DEV))
    np.testing.assert_array_equal(out.cpu().numpy(), g["d3pm_out"])


# --------------------------------------------------------------------------- decoder
MATHS = ["split16", "bf16x3", "f32"]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["decoder_4x6.npz", "decoder_ragged.npz"])
def test_decoder_forward(model1000, golden, name, cn, math):
    model1000.decoder.set_math(math)
    g = golden(name)
    sd = model1000.decoder.state_dict()
    assert weights_crc({k: v.cpu() for k, v in sd.items()}) == int(g["weights_crc"])
    nat = torch.from_numpy(g["natoms"])
    B = len(nat)
    te = model1000.time_embed(torch.full((B,), int(g["t"]), dtype=torch.long)).to(DEV)
    out = model1000.decoder(atom_types=torch.from_numpy(g["atom_types"]).to(DEV),
                            frac_coords=torch.from_numpy(g["frac"]).to(DEV),
                            lattices=torch.from_numpy(g["lattices"]).to(DEV), num_atoms=nat.to(DEV),
                            node2graph=torch.arange(B).repeat_interleave(nat).to(DEV), t=te,
                            text_embeds=cn[0].expand(B, -1).to(DEV))
    close(out.node_features.cpu(), g["node_features"], what="node_features")
    close(out.atom_types_out.cpu(), g["types"], what="types")
    close(out.coords_out.cpu(), g["coords"], what="coords")
    close(out.lattice_out.cpu(), g["lattice_out"], what="lattice")


def test_cfg_pair(model1000, golden, cn):
    g = golden("decoder_4x6.npz")
    nat = torch.from_numpy(g["natoms"])
    B = len(nat)
    te = model1000.time_embed(torch.full((B,), int(g["t"]), dtype=torch.long)).to(DEV)
    pa, pl, px = model1000.model_predictions(te, torch.from_numpy(g["atom_types"]).to(DEV),
                                             torch.from_numpy(g["frac"]).to(DEV),
                                             torch.from_numpy(g["lattices"]).to(DEV), nat.to(DEV), None, 2.0,
                                             cn[0].expand(B, -1).to(DEV), cn[1].expand(B, -1).to(DEV))
    close(pa.cpu(), g["cfg_types"], what="cfg types")
    close(pl.cpu(), g["cfg_lattice"], what="cfg lattice")
    close(px.cpu(), g["cfg_coords"], what="cfg coords")


# --------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("tag", ["64x20", "16x40"])
def test_teacher_forced_steps(model1000, golden, cn, tag, math):
    """Reference state at t + the reference's noise stream -> state at t-1."""
    model1000.decoder.set_math(math)
    g = golden(f"step_{tag}.npz")
    nat = g["natoms"].tolist()
    B, N = len(nat), sum(nat)
    for t in g["ts"]:
        t = int(t)
        torch.manual_seed(5000 + t)
        nz = None
        if t > 1:
            nz = (torch.rand((N, 104)), torch.randn(B, 3, 3), torch.randn(N, 3), torch.randn(N, 3))
        a, x, lat = model1000.reverse_step(t, torch.from_numpy(g[f"t{t}_a"]), torch.from_numpy(g[f"t{t}_x"]),
                                           torch.from_numpy(g[f"t{t}_l"]), nat, 2.0, 1e-5, cn[0], cn[1],
                                           noise=nz if nz is not None else None)
        np.testing.assert_array_equal(a.cpu().numpy(), g[f"t{t}_a_out"], err_msg=f"atom types t={t}")
        periodic_close(x.cpu(), g[f"t{t}_x_out"], what=f"frac t={t}")
        close(lat.cpu(), g[f"t{t}_l_out"], what=f"lattice t={t}")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("tag", ["256x40", "64x40", "c4chunk256", "512x40"])
def test_teacher_forced_steps_at_size(model1000, golden, cn, tag):
    """BASELINE sizes, one full reverse step each against the reference (fixtures written by the
    reference itself, tests/golden/make_golden.py steps_large): configs[2] (256 x 40), the per-GPU
    shard of configs[3] (64 x 40), configs[3] whole as one batch (512 x 40, the 1-GPU bench
    workload) and the first 256 crystals of configs[4]
    (natoms = randint(1, 81, seed 7)), which puts crystals of 1 to 80 atoms, segment tiles that
    span several small crystals and the gather path of the edge epilogues through the whole step.
    Same gates as test_teacher_forced_steps: types bit-exact (at t = 1 up to 2 fp32 near-ties of the
    logits' argmax, _t1_near_ties), |dx| <= 1e-4 periodic, lattices 1e-4."""
    g = golden(f"step_{tag}.npz")
    nat = g["natoms"].tolist()
    B, N = len(nat), sum(nat)
    if tag == "c4chunk256":
        full = torch.randint(1, 81, (2048,), generator=torch.Generator().manual_seed(7)).tolist()
        assert nat == full[:256] and min(nat) == 1 and max(nat) == 80
    for t in g["ts"]:
        t = int(t)
        torch.manual_seed(6000 + t)
        nz = None
        if t > 1:
            nz = (torch.rand((N, 104)), torch.randn(B, 3, 3), torch.randn(N, 3), torch.randn(N, 3))
        a, x, lat = model1000.reverse_step(t, torch.from_numpy(g[f"t{t}_a"].astype(np.int64)),
                                           torch.from_numpy(g[f"t{t}_x"]), torch.from_numpy(g[f"t{t}_l"]), nat,
                                           2.0, 1e-5, cn[0], cn[1], noise=nz)
        ref_a = g[f"t{t}_a_out"].astype(np.int64)
        flipped = np.nonzero(a.cpu().numpy() != ref_a)[0]
        ties = ""
        keep = np.ones(N, dtype=bool)
        if len(flipped):
            assert t == 1, f"{tag} t={t}: {len(flipped)} of {N} atom types differ"
            ties = _t1_near_ties(model1000, g, nat, cn, flipped, ref_a)
            # the corrector's decoder call reads the new types, so a crystal with a tie-broken type takes
            # another coordinate step: its atoms leave the coordinate comparison (the lattice update
            # precedes the types and stays compared for every crystal)
            n2g = np.repeat(np.arange(B), nat)
            keep = ~np.isin(n2g, n2g[flipped])
            ties += f"; {int((~keep).sum())} atoms of {len(np.unique(n2g[flipped]))} crystal(s) not compared"
        dx = periodic_close(x.cpu()[torch.from_numpy(keep)], g[f"t{t}_x_out"][keep], what=f"{tag} frac t={t}")
        dl = close(lat.cpu(), g[f"t{t}_l_out"], what=f"{tag} lattice t={t}")
        same = "bit-exact" if not len(flipped) else f"{N - len(flipped)} of"
        print(f"{tag} t={t}: types {same} ({N} atoms{ties}), max |dx| {dx:.2e}, lattice scaled err {dl:.2e}")


def _t1_near_ties(model, g, nat, cn, flipped, ref_a):
    """At t = 1 the types are the argmax of the CFG-mixed logits (no Gumbel noise, chemeleon.py:418 /
    diff_utils.py:286), so two classes whose logits agree to fp32 rounding are a tie that any other
    summation order may break the other way (512 x 40, atom 7124). Such a flip is accepted only for
    near-ties pinned on the REFERENCE's own logits: the fixture holds, per atom, the top-2 classes, the
    top-2 gap and the max |logit| of the reference's mixed logits at t = 1 (make_golden.py gen_t1_logits).
    At most 2 atoms; for each, the reference's gap <= 1e-5 of its logit scale, the device's gap likewise,
    and the device's class is the reference's second choice. Returns the note printed with the step."""
    assert len(flipped) <= 2, f"t=1: {len(flipped)} atom types differ"
    assert "t1_ref_gap" in g, "fixture lacks the reference's t = 1 logits (make_golden.py t1_logits)"
    B = len(nat)
    nat_t = torch.tensor(nat)
    te = model.time_embed(torch.full((B,), 1, dtype=torch.long)).to(DEV)
    kw = dict(atom_types=torch.from_numpy(g["t1_a"].astype(np.int64)).to(DEV),
              frac_coords=torch.from_numpy(g["t1_x"]).to(DEV), lattices=torch.from_numpy(g["t1_l"]).to(DEV),
              num_atoms=nat_t.to(DEV), node2graph=torch.arange(B).repeat_interleave(nat_t).to(DEV), t=te)
    pc = model.decoder(text_embeds=cn[0].expand(B, -1).to(DEV), **kw).atom_types_out
    pn = model.decoder(text_embeds=cn[1].expand(B, -1).to(DEV), **kw).atom_types_out
    mixed = ((1 - 2.0) * pn + 2.0 * pc).cpu()
    notes = []
    for i in flipped.tolist():
        top = torch.topk(mixed[i], 2)
        gap = float(top.values[0] - top.values[1])
        scale = float(mixed[i].abs().max())
        rgap, rscale = float(g["t1_ref_gap"][i]), float(g["t1_ref_scale"][i])
        rtop = [int(c) for c in g["t1_ref_top2"][i]]
        assert rtop[0] == int(ref_a[i])
        assert rgap <= 1e-5 * rscale, \
            f"t=1 atom {i}: the reference's top-2 gap {rgap:.2e} (scale {rscale:.2f}) is no near-tie"
        assert gap <= 1e-5 * scale, f"t=1 atom {i}: device top-2 gap {gap:.2e} of scale {scale:.2f}"
        assert top.indices.tolist() == rtop[::-1], \
            f"t=1 atom {i}: device top-2 {top.indices.tolist()} is not the reference's {rtop} swapped"
        notes.append(f"atom {i} reference gap {rgap:.1e} (scale {rscale:.2f}), device gap {gap:.1e}")
    return "; near-tie flips: " + ", ".join(notes)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("math", ["split16", "f32"])
def test_t1_step_512x40_math(model1000, golden, cn, math):
    """configs[3] as one batch, t = 1 (the argmax step) in the shipped split16 arithmetic and in exact
    fp32 MFMA arithmetic: which atoms' types differ from the reference (printed), under the gate of
    _t1_near_ties."""
    model1000.decoder.set_math(math)
    g = golden("step_512x40.npz")
    nat = g["natoms"].tolist()
    a, x, lat = model1000.reverse_step(1, torch.from_numpy(g["t1_a"].astype(np.int64)), torch.from_numpy(g["t1_x"]),
                                       torch.from_numpy(g["t1_l"]), nat, 2.0, 1e-5, cn[0], cn[1], noise=None)
    ref_a = g["t1_a_out"].astype(np.int64)
    flipped = np.nonzero(a.cpu().numpy() != ref_a)[0]
    note = _t1_near_ties(model1000, g, nat, cn, flipped, ref_a) if len(flipped) else ""
    rg = g["t1_ref_gap"] / g["t1_ref_scale"]
    print(f"512x40 t=1 {math}: {len(flipped)} of {len(ref_a)} atom types differ from the reference "
          f"(atoms {flipped.tolist()}){note}; the reference's smallest relative top-2 gaps: "
          f"{', '.join(f'atom {i} {rg[i]:.1e}' for i in np.argsort(rg)[:3])}")


@pytest.mark.parametrize("nat", [[40] * 64, [20] * 48, [80] * 9, [1] * 300 + [2] * 70 + [3] * 9,
                                 [23, 7, 40, 1, 80] * 23, [5, 9, 3, 12, 7, 1, 20]])
def test_edge_row_tiles_are_bit_identical(cn, nat):
    """Edge layer 2 on row tiles of exactly 256 edge rows (default; option 'edge_rows'): a node cut at
    a tile end keeps one sequential sum over its edges (the previous tile publishes its partial sum,
    the next continues it, or finishes it from the continued rows left in msgbuf when the partial was
    not there in time). One reverse step must agree bit for bit with node-aligned segment tiles, with
    the waiting path and with the msgbuf path forced ('edge_rows_nowait'). Shapes: 64 x 40 (400 row tiles, above
    'edge_layer_min': with 'edge_pairs' off the directed edge layers still run as two launches), crystals of 20
    and 80 atoms, runs of 1-3-atom crystals (up to 256 nodes per tile), ragged 1-80, a small mixed batch."""
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(12)
    a0 = torch.randint(0, 100, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    nz = (torch.rand((N, 104), generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
          torch.randn(N, 3, generator=g))
    model = _model(1000)
    model.decoder.set_option("edge_pairs", 0)  # (the directed edge-layer-1 schedules under test)
    outs = []
    _lib.prof_events(reset=True)
    for rows, nowait in ((0, 0), (1, 0), (1, 1), (1, 0)):
        model.decoder.set_option("edge_rows", rows)
        model.decoder.set_option("edge_rows_nowait", nowait)
        outs.append([o.cpu() for o in model.reverse_step(500, a0, x0, l0, nat, 2.0, 1e-5, cn[0], cn[1], noise=nz)])
    torch.cuda.synchronize()
    ev = _lib.prof_events()
    del model
    torch.cuda.empty_cache()
    assert ev["layer_wait_timeouts"] == 0 and ev["tail_wait_timeouts"] == 0, ev
    for k, name in ((1, "row tiles"), (2, "row tiles, msgbuf path"), (3, "row tiles, second run")):
        for u, v, what in zip(outs[0], outs[k], ("types", "frac", "lattice")):
            assert torch.equal(u, v), f"{what}: {name} differ from node-aligned segment tiles"


@pytest.mark.parametrize("nat", [[40] * 64, [23, 7, 40, 1, 80] * 23])
def test_presplit_node_gemms_match_in_loop_split(cn, nat):
    """split16 node GEMMs reading their A operands pre-split by the producing kernels (option 'node_ps', off by
    default since it measured no faster: film_ln, embed, the segment-mean epilogue and the node GEMM epilogues
    write split rows scaled per
    128-column chunk; the GEMM rescales its accumulators at chunk boundaries) against the in-loop register
    split of round 3 (per-row scales): same types, coordinates and lattices to fp32-rounding level (the two
    differ only in where the power-of-two scales change), and the decoder outputs within 8e-6 scaled (the
    bound test_math_modes_agree puts between split16 and exact fp32)."""
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(15)
    a0 = torch.randint(0, 100, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    nz = (torch.rand((N, 104), generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
          torch.randn(N, 3, generator=g))
    model = _model(1000)
    te = model.time_embed(torch.full((B,), 300, dtype=torch.long)).to(DEV)
    nat_t = torch.tensor(nat)
    steps, decs = [], []
    for ps in (1, 0):
        model.decoder.set_option("node_ps", ps)
        steps.append([o.cpu() for o in model.reverse_step(500, a0, x0, l0, nat, 2.0, 1e-5, cn[0], cn[1], noise=nz)])
        o = model.decoder(atom_types=a0.to(DEV), frac_coords=x0.to(DEV), lattices=l0.to(DEV), num_atoms=nat_t.to(DEV),
                          node2graph=torch.arange(B).repeat_interleave(nat_t).to(DEV), t=te,
                          text_embeds=cn[0].expand(B, -1).to(DEV))
        decs.append([o.node_features.cpu(), o.atom_types_out.cpu(), o.coords_out.cpu(), o.lattice_out.cpu()])
    del model
    torch.cuda.empty_cache()
    assert torch.equal(steps[0][0], steps[1][0]), "atom types differ between the two node-GEMM forms"
    dx = periodic_close(steps[0][1], steps[1][1], tol=1e-5, what="frac")
    dl = close(steps[0][2], steps[1][2], rtol=1e-5, what="lattice")
    errs = [close(u, v, rtol=8e-6, what=w) for u, v, w in zip(decs[0], decs[1], ("node", "types", "coords", "lattice"))]
    print(f"pre-split vs in-loop split: step |dx| {dx:.2e}, lattice {dl:.2e}; decoder scaled errors "
          + ", ".join(f"{e:.1e}" for e in errs))


@pytest.mark.timeout(300)
def test_ragged_2048_full_size_step(model1000, cn):
    """configs[4] at full size on one GPU (2048 crystals, natoms = randint(1, 81, seed 7),
    Sum n^2 = 4.4 M edges per decoder call): one perf-mode step from pure noise and one at
    t = 500 are finite and in range, and a crystal's result does not depend on the batch it
    is sampled in (its slice of the 2048 batch equals the same crystals sampled alone)."""
    nat = torch.randint(1, 81, (2048,), generator=torch.Generator().manual_seed(7)).tolist()
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(8)
    a = torch.randint(0, 104, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    lat = torch.randn(B, 3, 3, generator=g) * 3 * model1000.mask_lattice_matrix
    for t in (1000, 500):
        a2, x2, l2 = model1000.reverse_step(t, a, x, lat, nat, 2.0, 1e-5, cn[0], cn[1], noise=None, seed=3)
        assert torch.isfinite(x2).all() and torch.isfinite(l2).all()
        assert ((a2 >= 0) & (a2 < 104)).all()
        assert ((x2 >= 0) & (x2 <= 1)).all()
        if t == 1000:
            assert (l2.abs() <= 6).all()
    # the last 5 crystals alone (node_base / graph_base keep the Philox keys global)
    g0 = B - 5
    n0 = sum(nat[:g0])
    sub = model1000.reverse_step(500, a[n0:], x[n0:], lat[g0:], nat[g0:], 2.0, 1e-5, cn[0], cn[1], noise=None,
                                 seed=3, node_base=n0, graph_base=g0)
    assert torch.equal(sub[0], a2[n0:]) and torch.equal(sub[1], x2[n0:]) and torch.equal(sub[2], l2[g0:])


def _lattice_errors(lat, ref):
    """element-wise relative error (floored at 1e-3 of the state's largest entry)
    and normwise error (max abs error / max |entry|, per state)"""
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=(1, 2, 3), keepdims=True) * 1e-3)
    el = float((np.abs(lat - ref) / scale).max())
    nw = float((np.abs(lat - ref).max(axis=(1, 2, 3)) / np.abs(ref).max(axis=(1, 2, 3))).max())
    return el, nw


def _trajectory_errors(model, g, cn, T):
    torch.manual_seed(42)
    states = list(model.sample_states([6] * 4, None, 2.0, 1e-5, noise="torch", text_embeds=cn[0],
                                      null_text_embeds=cn[1], clone=True))
    by_t = {s[0]: s for s in states}
    ts = [int(t) for t in g["t"]]
    a = np.stack([by_t[t][1].cpu().numpy() for t in ts])
    x = np.stack([by_t[t][2].cpu().numpy() for t in ts])
    lat = np.stack([by_t[t][3].cpu().numpy() for t in ts])
    flips = int((a != g["atom_types"]).sum())
    dx = periodic_close(x, g["frac"], tol=1.0)
    el, nw = _lattice_errors(lat, g["lattices"])
    msg = (f"T={T} {model.decoder.get_math()}: atom-type flips {flips}/{a.size}, max |dx| {dx:.2e}, "
           f"lattice element-wise {el:.2e}, normwise {nw:.2e}")
    if "lattices_1thread" in g:
        rel, rnw = _lattice_errors(g["lattices_1thread"], g["lattices"])
        rdx = periodic_close(g["frac_1thread"], g["frac"], tol=1.0)
        msg += f" | reference 1 vs {int(g['threads'])} threads: |dx| {rdx:.2e}, element-wise {rel:.2e}, normwise {rnw:.2e}"
    print(msg)
    return a, x, lat, flips, dx, el, nw


@pytest.mark.parametrize("math", MATHS)
def test_trajectory_c0(model100, golden, cn, math):
    """C0 (configs[0]): 4 x 6 atoms, T = 100, seed 42, the full sampler."""
    model100.decoder.set_math(math)
    g = golden("trajectory_4x6_T100.npz")
    a, x, lat, flips, dx, el, nw = _trajectory_errors(model100, g, cn, 100)
    np.testing.assert_array_equal(a, g["atom_types"])
    assert dx <= 1e-4
    close(lat, g["lattices"], what="trajectory lattices")


@pytest.mark.parametrize("math", MATHS)
def test_trajectory_c0_1000_steps(model1000, golden, cn, math):
    """4 x 6 atoms, the full 1000-step sampler (every 10th state compared),
    seed 42, reference CPU trajectory. Over 1000 reverse DDPM steps the lattice
    grows ~10^4x and relative error in small entries is amplified: the
    reference itself, re-run single-threaded, differs from its 8-thread run by
    ~2e-4 element-wise (~1e-6 normwise; stored in the fixture and printed).
    Gate: atom types bit-exact, |dx| <= 1e-4, lattice normwise <= 1e-4."""
    model1000.decoder.set_math(math)
    g = golden("trajectory_4x6_T1000.npz")
    a, x, lat, flips, dx, el, nw = _trajectory_errors(model1000, g, cn, 1000)
    np.testing.assert_array_equal(a, g["atom_types"])
    assert dx <= 1e-4, dx
    assert nw <= 1e-4, nw


@pytest.mark.timeout(600)
def test_trajectory_64x20_1000_steps(model1000, golden, cn):
    """configs[1] (64 x 20 atoms, T = 1000, seed 42): the whole sampler in parity mode (noise='torch', the
    reference's CPU RNG stream, captured step replayed per t) against the unmodified reference's own
    trajectory (tests/golden/make_golden.py trajectory64x20: every 50th state and the final one,
    reference chemeleon.py:379-467). About 1.3 M Gumbel-argmax decisions: a logit difference at fp32
    rounding level can flip one of them, after which that crystal follows another trajectory. Gate:
    atom-type flips touch at most 2 of the 64 crystals (listed); every crystal without a flip keeps
    its types bit-exact in every stored state, |dx| <= 1e-4 (periodic) and its lattice within 1e-4
    normwise (max abs error / max |entry| of that crystal's lattice, per state)."""
    g = golden("trajectory_64x20_T1000.npz")
    want = set(int(t) for t in g["t"])
    torch.manual_seed(42)
    got = {}
    for st in model1000.sample_states([20] * 64, None, 2.0, 1e-5, noise="torch", text_embeds=cn[0],
                                      null_text_embeds=cn[1], clone=False):
        if st[0] in want:
            got[st[0]] = [v.cpu().numpy().copy() for v in st[1:]]
    gate_64x20(got, g)


def gate_64x20(got, g, label="64x20 T=1000"):
    """The reference gate of test_trajectory_64x20_1000_steps on {t: (atom_types, frac, lattices)} of
    the stored timesteps (also used by the sample-parallel run, tests/test_gpu_distributed.py)."""
    ts = [int(t) for t in g["t"]]
    nat = [20] * 64
    assert sorted(got) == sorted(ts)
    a = np.stack([got[t][0] for t in ts])
    x = np.stack([got[t][1] for t in ts])
    lat = np.stack([got[t][2] for t in ts])
    ra, rx, rl = g["atom_types"].astype(np.int64), g["frac"], g["lattices"]
    B = len(nat)
    flip = (a != ra).reshape(len(ts), B, 20).any(axis=(0, 2))  # crystals with any type flip
    first = {b: ts[int(np.argmax((a != ra).reshape(len(ts), B, 20)[:, b].any(axis=1)))] for b in np.nonzero(flip)[0]}
    clean = ~flip
    d = np.abs(x - rx).reshape(len(ts), B, 20, 3)
    d = np.minimum(d, 1.0 - d)
    dx = float(d[:, clean].max()) if clean.any() else 0.0
    nw = (np.abs(lat - rl).max(axis=(2, 3)) / np.maximum(np.abs(rl).max(axis=(2, 3)), 1e-30))  # [state, crystal]
    lnw = float(nw[:, clean].max()) if clean.any() else 0.0
    print(f"{label}: crystals with an atom-type flip {int(flip.sum())}/{B} (first stored flip at t: {first}); "
          f"clean crystals: max |dx| {dx:.2e}, lattice normwise {lnw:.2e}; all crystals: max |dx| {float(d.max()):.2e}")
    assert flip.sum() <= 2, f"atom-type flips in {int(flip.sum())} crystals: {first}"
    assert dx <= 1e-4, dx
    assert lnw <= 1e-4, lnw


def test_decoder_large_ragged_vs_oracle(model1000, cn):
    """Crystals from 1 to 80 atoms (stress-config sizes) in one batch, both
    conditionings, against the CPU oracle."""
    nat = [80, 1, 37, 64, 2, 80, 13]
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(17)
    a = torch.randint(0, 104, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    lat = torch.randn(B, 3, 3, generator=g) * 4
    te = model1000.time_embed(torch.full((B,), 321, dtype=torch.long))
    sd = {k: v.detach().cpu() for k, v in model1000.decoder.state_dict().items()}
    nat_t = torch.tensor(nat)
    n2g = torch.arange(B).repeat_interleave(nat_t)
    for math in MATHS:
        model1000.decoder.set_math(math)
        types, latt, coords, nodes = model1000.decoder.forward_cfg(a.to(DEV), x.to(DEV), lat.to(DEV), nat_t.to(DEV),
                                                                   te.to(DEV), cn[0].expand(B, -1).to(DEV),
                                                                   cn[1].expand(B, -1).to(DEV), need_nodes=True)
        for c, text in enumerate(cn):
            rt, rl, rc, rh = O.cspnet_forward(sd, default_config(), a, x, lat, nat_t, n2g, te, text.expand(B, -1))
            close(nodes[c].cpu(), rh, what=f"{math} nodes c={c}")
            close(types[c].cpu(), rt, what=f"{math} types c={c}")
            close(coords[c].cpu(), rc, what=f"{math} coords c={c}")
            close(latt[c].cpu(), rl, what=f"{math} lattice c={c}")


def test_decoder_above_128_atoms_vs_oracle(model1000, cn):
    """Crystals of 129 and 97 atoms between 1 and 3 (the reference workload stops at 80; a fully connected batch
    takes up to 256), both conditionings, against the CPU oracle under the tolerance of
    test_decoder_large_ragged_vs_oracle. Which schedule ran is read from the profiling counters and asserted: at
    its 102 row tiles the batch is below edge_layer_min (256), so every math mode's default is the two-launch form
    (no one-grid launch recorded); split16 then runs once more with edge_layer_min 1, where the pair grid must
    record one launch per layer. There the 129-atom crystal's last row tile reads 66 pair tiles, so its jobs'
    flag polling takes its second pass; no wait may time out, no job be repaired or find another XCD's tiles."""
    nat = [129, 1, 97, 3]
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(23)
    a = torch.randint(0, 104, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    lat = torch.randn(B, 3, 3, generator=g) * 4
    te = model1000.time_embed(torch.full((B,), 321, dtype=torch.long))
    dec = model1000.decoder
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    nat_t = torch.tensor(nat)
    n2g = torch.arange(B).repeat_interleave(nat_t)
    refs = [O.cspnet_forward(sd, default_config(), a, x, lat, nat_t, n2g, te, text.expand(B, -1)) for text in cn]
    L = default_config()["num_layers"]
    lib = _lib.load()
    _lib.check(lib.chm_prof_enable(1), "chm_prof_enable")
    try:
        for math, layer_min, want_grid in [(m, 256, 0) for m in MATHS] + [("split16", 1, L)]:
            dec.set_math(math)
            dec.set_option("edge_layer_min", layer_min)
            _lib.prof_events(reset=True)
            _lib.check(lib.chm_prof_reset(), "chm_prof_reset")
            types, latt, coords, nodes = dec.forward_cfg(a.to(DEV), x.to(DEV), lat.to(DEV), nat_t.to(DEV), te.to(DEV),
                                                         cn[0].expand(B, -1).to(DEV), cn[1].expand(B, -1).to(DEV),
                                                         need_nodes=True)
            torch.cuda.synchronize()
            ev = _lib.prof_events()
            n_grid, n_two = _lib.prof_read(_lib.K_EDGE_LAYER)[0], _lib.prof_read(_lib.K_EDGE_MESSAGE)[0]
            what = f"{math} edge_layer_min {layer_min}"
            print(f"{what}: {n_grid} one-grid launches, {n_two} layer-2 launches of the two-launch form; events {ev}")
            assert n_grid == want_grid and n_two == L - want_grid, (what, n_grid, n_two)
            assert ev["layer_wait_timeouts"] == 0 and ev["layer_repairs"] == 0 and ev["layer_other_xcd"] == 0, (what, ev)
            for c, (rt, rl, rc, rh) in enumerate(refs):
                close(nodes[c].cpu(), rh, what=f"{what} nodes c={c}")
                close(types[c].cpu(), rt, what=f"{what} types c={c}")
                close(coords[c].cpu(), rc, what=f"{what} coords c={c}")
                close(latt[c].cpu(), rl, what=f"{what} lattice c={c}")
    finally:
        dec.set_option("edge_layer_min", 256)  # (the default)
        lib.chm_prof_enable(0)
        lib.chm_prof_reset()


@pytest.mark.parametrize("lat_scale", [300.0, 3000.0])
def test_decoder_wide_range_vs_oracle(model1000, cn, lat_scale):
    """Lattices 300x / 3000x the usual scale (vec(LL^T) up to ~1e8): the lattice term reaches P,
    S, agg, the node MLP and the residual stream (up to ~1e6 / 1e7 after six layers), far outside
    fp16's range. The split16 node GEMMs scale each A row by its
    max (written by the producing kernels), so every arithmetic stays finite and within 1e-4 of
    the CPU oracle."""
    nat = [12, 5, 20, 1, 9]
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(29)
    a = torch.randint(0, 104, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    lat = torch.randn(B, 3, 3, generator=g) * 4 * lat_scale
    te = model1000.time_embed(torch.full((B,), 700, dtype=torch.long))
    sd = {k: v.detach().cpu() for k, v in model1000.decoder.state_dict().items()}
    nat_t = torch.tensor(nat)
    n2g = torch.arange(B).repeat_interleave(nat_t)
    hid = []
    ref = [O.cspnet_forward(sd, default_config(), a, x, lat, nat_t, n2g, te, text.expand(B, -1), hidden=hid)
           for text in cn]
    assert max(float(h.abs().max()) for h in hid) > 65504  # the residual stream does leave fp16's range
    for math in MATHS:
        model1000.decoder.set_math(math)
        types, latt, coords, nodes = model1000.decoder.forward_cfg(a.to(DEV), x.to(DEV), lat.to(DEV), nat_t.to(DEV),
                                                                   te.to(DEV), cn[0].expand(B, -1).to(DEV),
                                                                   cn[1].expand(B, -1).to(DEV), need_nodes=True)
        for c in range(2):
            rt, rl, rc, rh = ref[c]
            close(nodes[c].cpu(), rh, what=f"{math} nodes c={c} x{lat_scale}")
            close(types[c].cpu(), rt, what=f"{math} types c={c} x{lat_scale}")
            close(coords[c].cpu(), rc, what=f"{math} coords c={c} x{lat_scale}")
            close(latt[c].cpu(), rl, what=f"{math} lattice c={c} x{lat_scale}")
    model1000.decoder.set_math("split16")


@pytest.mark.parametrize("t", [500, 1000])
def test_math_modes_agree(model1000, cn, t):
    """The GEMM arithmetics agree to fp32 rounding level on 64 x 20, for the
    CFG pair (P = 2) and for a single conditioning (P = 1)."""
    nat = [20] * 64
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(23)
    a = torch.randint(0, 104, (N,), generator=g).to(DEV)
    x = torch.rand(N, 3, generator=g).to(DEV)
    lat = (torch.randn(B, 3, 3, generator=g) * 4).to(DEV)
    te = model1000.time_embed(torch.full((B,), t, dtype=torch.long)).to(DEV)
    nat_t = torch.tensor(nat).to(DEV)
    n2g = torch.arange(B).repeat_interleave(nat_t.cpu()).to(DEV)
    outs, single = {}, {}
    for math in MATHS:
        model1000.decoder.set_math(math)
        outs[math] = model1000.decoder.forward_cfg(a, x, lat, nat_t, te, cn[0].expand(B, -1).to(DEV),
                                                   cn[1].expand(B, -1).to(DEV), need_nodes=True)
        single[math] = model1000.decoder(a, x, lat, nat_t, n2g, t=te, text_embeds=cn[0].expand(B, -1).to(DEV))
    model1000.decoder.set_math("split16")
    errs = {}
    for m in ("split16", "bf16x3"):
        for k, name in enumerate(["types", "lattice", "coords", "nodes"]):
            for c in range(2):
                e = scaled_err(outs[m][k][c].cpu(), outs["f32"][k][c].cpu())
                errs[(m, "pair", c, name)] = (e.max(), np.median(e))
            e = scaled_err(single[m][k].cpu(), single["f32"][k].cpu())
            errs[(m, "single", 0, name)] = (e.max(), np.median(e))
    for key, (e, med) in errs.items():
        print(f"t={t} {key}: scaled err vs f32 max {e:.2e} median {med:.2e}")
    bad = {k: e for k, (e, med) in errs.items() if e > 2e-5}
    assert not bad, f"math modes disagree: {bad}"


def test_sample_api_returns_sorted_structures(model100, golden, cn):
    torch.manual_seed(42)
    atoms = model100.sample(None, 6, 4, text_embeds=cn[0], null_text_embeds=cn[1])
    g = golden("trajectory_4x6_T100.npz")
    nums = np.concatenate([np.asarray(at.numbers) for at in atoms])
    np.testing.assert_array_equal(nums, g["final_sorted_numbers"])


# --------------------------------------------------------------------------- perf-mode properties
def test_philox_shard_invariance(model100, cn):
    """Perf-mode noise is keyed by global indices: sampling 6 crystals as one
    batch or as two shards gives identical results."""
    nat = [5, 9, 3, 12, 7, 4]
    full = list(model100.sample_states(nat, None, 2.0, 1e-5, noise="philox", seed=7, text_embeds=cn[0],
                                       null_text_embeds=cn[1], clone=False, t_stop=90))[-1]
    g = torch.Generator().manual_seed(7)
    l0 = torch.randn(6, 3, 3, generator=g) * model100.mask_lattice_matrix
    x0 = torch.randn(sum(nat), 3, generator=g)
    parts = []
    for (g0, g1) in ((0, 2), (2, 6)):
        n0, n1 = sum(nat[:g0]), sum(nat[:g1])
        parts.append(list(model100.sample_states(nat[g0:g1], None, 2.0, 1e-5, noise="philox", seed=7,
                                                 text_embeds=cn[0], null_text_embeds=cn[1], clone=False,
                                                 t_stop=90, node_base=n0, graph_base=g0,
                                                 init=(l0[g0:g1], x0[n0:n1])))[-1])
    for k in (1, 2, 3):
        cat = torch.cat([p[k] for p in parts])
        assert torch.equal(cat, full[k]), f"state {k} differs between 1 and 2 shards"


@pytest.mark.parametrize("nat,lanes", [pytest.param([5, 9, 3, 12, 7, 1, 20], k, id=str(k)) for k in (1, 2, 3)]
                         + [pytest.param([130, 3, 90], 1, id="130-3-90-1")])
def test_graph_replay_matches_eager(model100, cn, nat, lanes):
    """One captured reverse step replayed per timestep (device-side t) gives
    bit-identical states to eager stepping, also with the crystals split over
    concurrent stream lanes inside the graph, and (one lane) with crystals of 130 and 90 atoms."""
    runs = []
    for graph in (False, True):
        states = list(model100.sample_states(nat, None, 2.0, 1e-5, noise="philox", seed=11, text_embeds=cn[0],
                                             null_text_embeds=cn[1], clone=True, graph=graph, t_stop=80,
                                             lanes=lanes))
        runs.append(states)
    assert [s[0] for s in runs[0]] == [s[0] for s in runs[1]]
    for se, sg in zip(*runs):
        for k in (1, 2, 3):
            assert torch.equal(se[k], sg[k]), f"t={se[0]} state {k}"


def test_pair_grid_graph_replay_matches_eager(cn):
    """The static pair grid (the default from 256 row tiles) inside captured step graphs: replays give the
    eager states bit for bit, and no layer-2 job finds its pair tiles written on another XCD, times out or is
    repaired. (The grid's block -> XCD rotation is not anchored at XCD 0 under graph replay: an absolute XCD
    check flagged every job there while the eager tests saw none; the check is relative since.)"""
    model = _model(100)
    nat = [40] * 64  # 400 row tiles
    runs, events = [], []
    for graph in (False, True):
        _lib.prof_events(reset=True)
        runs.append(list(model.sample_states(nat, None, 2.0, 1e-5, noise="philox", seed=13, text_embeds=cn[0],
                                             null_text_embeds=cn[1], clone=True, graph=graph, t_stop=96)))
        torch.cuda.synchronize()
        events.append(_lib.prof_events())
    del model
    torch.cuda.empty_cache()
    print("events (eager, graph):", events)
    for ev in events:
        assert ev["layer_other_xcd"] == 0 and ev["layer_wait_timeouts"] == 0 and ev["layer_repairs"] == 0
    assert [s[0] for s in runs[0]] == [s[0] for s in runs[1]]
    for se, sg in zip(*runs):
        for k in (1, 2, 3):
            assert torch.equal(se[k], sg[k]), f"t={se[0]} state {k}"


def test_torch_noise_graph_matches_eager(model100, cn):
    """Parity mode (noise='torch', the reference's CPU RNG stream) under the captured step: every
    step's draws go through pinned host buffers into fixed device buffers before the replay. The
    whole T = 100 trajectory (down to t = 0, where no noise is drawn) equals eager stepping bit for
    bit, and the CPU generator ends in the same state."""
    nat = [5, 9, 3, 12, 7, 1, 20]
    runs, after = [], []
    for graph in (False, True):
        torch.manual_seed(1234)
        runs.append(list(model100.sample_states(nat, None, 2.0, 1e-5, noise="torch", text_embeds=cn[0],
                                                null_text_embeds=cn[1], clone=True, graph=graph)))
        after.append(torch.rand(4))
    assert [s[0] for s in runs[0]] == [s[0] for s in runs[1]] and runs[0][-1][0] == 0
    for se, sg in zip(*runs):
        for k in (1, 2, 3):
            assert torch.equal(se[k], sg[k]), f"t={se[0]} state {k}"
    assert torch.equal(after[0], after[1]), "the CPU generator consumed a different number of draws"


def test_large_batch_step_is_finite(model1000, cn):
    """512 x 40 (BASELINE metric shape): one reverse step in perf mode."""
    nat = [40] * 512
    N = sum(nat)
    a = torch.zeros(N, dtype=torch.long)
    x = torch.rand(N, 3, generator=torch.Generator().manual_seed(1))
    lat = torch.randn(512, 3, 3, generator=torch.Generator().manual_seed(2)) * model1000.mask_lattice_matrix
    a2, x2, l2 = model1000.reverse_step(1000, a, x, lat, nat, 2.0, 1e-5, cn[0], cn[1], noise=None, seed=3)
    assert torch.isfinite(x2).all() and torch.isfinite(l2).all()
    assert ((a2 >= 0) & (a2 < 104)).all()
    assert ((x2 >= 0) & (x2 <= 1)).all()
    assert (l2.abs() <= 6).all()  # t == T clip


# --------------------------------------------------------------------------- edge layer 1 on pairs
@pytest.mark.parametrize("nat", [[3, 5, 8, 1, 40, 17, 2, 80], [40] * 64, [130, 3, 90]])
def test_edge_pairs_match_directed_edges(model1000, cn, nat):
    """Option edge_pairs: edge layer 1 once per unordered pair (the reverse edge's Fourier features are the
    forward ones with the sine half negated). Its decoder outputs agree with the directed form to within fp32
    rounding of the features (the reference's two argument roundings differ by up to 8e-5 on the k = 127
    features; measured on the CPU oracle: 2e-6 of the outputs' scale), i.e. far inside the 1e-4 gate."""
    dec = model1000.decoder
    g = torch.Generator().manual_seed(11)
    N, B = sum(nat), len(nat)
    a = torch.randint(0, 100, (N,), generator=g).to(DEV)
    x = torch.rand(N, 3, generator=g).to(DEV)
    lat = (torch.randn(B, 3, 3, generator=g) + 4 * torch.eye(3)).to(DEV)
    te = model1000.time_embed(torch.full((B,), 437, dtype=torch.long)).to(DEV)
    c, n = cn[0].expand(B, -1).to(DEV), cn[1].expand(B, -1).to(DEV)
    outs = []
    for on in (0, 1):
        dec.set_option("edge_pairs", on)
        outs.append([o.cpu() for o in dec.forward_cfg(a, x, lat, nat, te, c, n, need_nodes=True)])
    dec.set_option("edge_pairs", 1)  # (the default)
    errs = [close(p, d, rtol=2e-5, what=f"edge_pairs {name}")
            for name, d, p in zip(("types", "lattice", "coords", "nodes"), *outs)]
    assert max(errs) > 0  # (the option really changed the arithmetic path)


@pytest.mark.parametrize("nat", [[40] * 64, [23, 7, 40, 1, 80] * 23, [1] * 300 + [2] * 70 + [3] * 9])
def test_edge_pairs_layer2_schedules_are_bit_identical(cn, nat):
    """With edge layer 1 on pairs (the default), edge layer 2's schedules stay bit-identical to one another:
    node-aligned segment tiles, row tiles, and row tiles with the msgbuf path forced ('edge_rows_nowait'),
    and the step is reproducible."""
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(16)
    a0 = torch.randint(0, 100, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    nz = (torch.rand((N, 104), generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
          torch.randn(N, 3, generator=g))
    model = _model(1000)
    model.decoder.set_option("edge_pairs", 1)
    outs = []
    for rows, nowait in ((0, 0), (1, 0), (1, 1), (1, 0)):
        model.decoder.set_option("edge_rows", rows)
        model.decoder.set_option("edge_rows_nowait", nowait)
        outs.append([o.cpu() for o in model.reverse_step(500, a0, x0, l0, nat, 2.0, 1e-5, cn[0], cn[1], noise=nz)])
    del model
    torch.cuda.empty_cache()
    for k in (1, 2, 3):
        for u, v, what in zip(outs[0], outs[k], ("types", "frac", "lattice")):
            assert torch.equal(u, v), f"{what}: edge-pairs layer-2 schedule {k} differs"


@pytest.mark.parametrize("nat", [[40] * 64, [23, 7, 40, 1, 80] * 23, [1] * 300 + [2] * 70 + [3] * 9, [40] * 512])
def test_edge_pairs_grid_is_bit_identical(cn, nat):
    """Both edge layers on pairs in one static grid (k_edge16_pairs_grid, option edge_pairs_layer = 1, the default
    from 256 row tiles): block 8 k + x runs job k of list x, layer-2 jobs wait on per-pair-tile flags of their
    list (3 row tiles here too: lists of XCDs without rows are empty). One reverse step
    equals the two-launch pair schedule bit for bit, also with the repair launches forced
    ('edge_layer_repair'); in the plain run no wait times out, no block runs on an unplanned XCD, nothing is
    repaired."""
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(19)
    a0 = torch.randint(0, 100, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    nz = (torch.rand((N, 104), generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
          torch.randn(N, 3, generator=g))
    model = _model(1000)
    model.decoder.set_option("edge_pairs", 1)
    model.decoder.set_option("edge_layer_min", 1)  # (the one-grid form for every shape here)
    outs, events = [], []
    for form, repair in ((0, 0), (1, 0), (1, 1)):
        model.decoder.set_option("edge_pairs_layer", form)
        model.decoder.set_option("edge_layer_repair", repair)
        _lib.prof_events(reset=True)
        outs.append([o.cpu() for o in model.reverse_step(500, a0, x0, l0, nat, 2.0, 1e-5, cn[0], cn[1], noise=nz)])
        torch.cuda.synchronize()
        events.append(_lib.prof_events())
    del model
    torch.cuda.empty_cache()
    print("events (two launches, static grid, forced repair):", events)
    assert events[1]["layer_wait_timeouts"] == 0 and events[1]["layer_other_xcd"] == 0
    assert events[1]["layer_repairs"] == 0
    assert events[2]["layer_repairs"] == 12  # 2 decoder pairs x 6 layers
    for k, name in ((1, "static grid"), (2, "static grid + forced repair")):
        for u, v, what in zip(outs[0], outs[k], ("types", "frac", "lattice")):
            assert torch.equal(u, v), f"{what}: {name} differs from the two-launch pair schedule"


@pytest.mark.parametrize("nat", [[40] * 64, [23, 7, 40, 1, 80] * 23, [1] * 300 + [2] * 70 + [3] * 9, [79, 78, 2, 80]])
def test_pair_epilogue_staged_rows_are_bit_identical(cn, nat):
    """The pair tiles' epilogue stages the P / Q rows of their nodes in LDS (both conditionings when they fit,
    else conditioning 0; tiles of more than 78 nodes read global memory): the same values in the same
    arithmetic, so one reverse step equals the unstaged form ('edge_pairs_pq_global') bit for bit, in the
    two-launch schedule and in the pair grid. The shapes mix tiles of one and two crystals, of 1-atom crystals,
    and of 78-80-atom crystals (staged and global at the size limit)."""
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(23)
    a0 = torch.randint(0, 100, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    nz = (torch.rand((N, 104), generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
          torch.randn(N, 3, generator=g))
    model = _model(1000)
    model.decoder.set_option("edge_pairs", 1)
    model.decoder.set_option("edge_layer_min", 1)
    outs = []
    for form, glob in ((0, 1), (0, 0), (1, 0)):
        model.decoder.set_option("edge_pairs_layer", form)
        model.decoder.set_option("edge_pairs_pq_global", glob)
        outs.append([o.cpu() for o in model.reverse_step(500, a0, x0, l0, nat, 2.0, 1e-5, cn[0], cn[1], noise=nz)])
    del model
    torch.cuda.empty_cache()
    for k, name in ((1, "two launches, staged"), (2, "pair grid, staged")):
        for u, v, what in zip(outs[0], outs[k], ("types", "frac", "lattice")):
            assert torch.equal(u, v), f"{what}: {name} differs from the unstaged pair epilogue"


@pytest.mark.parametrize("nat,nowait", [([20] * 64, 0), ([20] * 64, 1), ([6] * 4, 0), ([20] * 30, 0),
                                        ([190, 37, 5, 1, 80, 2, 64, 100], 0), ([190, 37, 5, 1, 80, 2, 64, 100], 1)])
def test_short_row_tiles_are_bit_identical(cn, nat, nowait):
    """Mixed row tiling (r6): a batch below edge_layer_min row tiles whose last round of 256-row tiles is at most 3/4
    full runs edge layer 2 as its 256-row tiles, then 192-row tiles (k_edge16_short) for that round's rows. A node cut
    at a tile end stays one sequential sum over its edges (published partial sum, or the continued rows through
    msgbuf: 'edge_rows_nowait'), so one reverse step equals the uniform tiling ('edge_rows_short' 0) bit for bit.
    Shapes: configs[1] (64 tiles of 256 + 48 of 192), all-short tilings of one partial round, and a ragged batch with
    a 190-atom crystal (nodes longer than half a short tile, cut at 256 / 192 boundaries)."""
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(29)
    a0 = torch.randint(0, 100, (N,), generator=g)
    x0 = torch.rand(N, 3, generator=g)
    l0 = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    nz = (torch.rand((N, 104), generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 3, generator=g),
          torch.randn(N, 3, generator=g))
    lib = _lib.load()
    arr = (ctypes.c_int32 * B)(*nat)
    want = lib.chm_debug_short_row_tiles(arr, B, 2, torch.cuda.get_device_properties(0).multi_processor_count, 256)
    assert want >= 0, "the shape should take a mixed tiling"
    model = _model(1000)
    model.decoder.set_option("edge_rows_nowait", nowait)
    outs, took = [], []
    for short in (0, 1):
        model.decoder.set_option("edge_rows_short", short)
        outs.append([o.cpu() for o in model.reverse_step(500, a0, x0, l0, nat, 2.0, 1e-5, cn[0], cn[1], noise=nz)])
        took.append([lib.chm_batch_short_row_tiles(b.handle) for b in model.decoder._batches.values()])
    del model
    torch.cuda.empty_cache()
    assert took[0] and all(t == -1 for t in took[0])
    assert took[1] and all(t == want for t in took[1]), (took[1], want)
    for u, v, what in zip(outs[0], outs[1], ("types", "frac", "lattice")):
        assert torch.equal(u, v), f"{what}: the mixed row tiling differs from the uniform one"


def test_short_row_tiles_single_conditioning_bit_identical(cn):
    """The mixed row tiling with one conditioning (a plain decoder call, max_pairs = 1: 2 jobs per row tile): 30
    crystals of 20 atoms take 63 tiles of 192 rows in one round; the decoder outputs equal the uniform tiling's."""
    nat = [20] * 30
    B, N = len(nat), sum(nat)
    g = torch.Generator().manual_seed(31)
    a = torch.randint(0, 104, (N,), generator=g)
    x = torch.rand(N, 3, generator=g)
    lat = torch.eye(3).expand(B, 3, 3) * 4.0 + 0.3 * torch.randn(B, 3, 3, generator=g)
    model = _model(1000)
    te = model.time_embed(torch.full((B,), 700, dtype=torch.long)).to(DEV)
    nat_t = torch.tensor(nat)
    lib = _lib.load()
    outs, took = [], []
    for short in (0, 1):
        model.decoder.set_option("edge_rows_short", short)
        o = model.decoder(atom_types=a.to(DEV), frac_coords=x.to(DEV), lattices=lat.to(DEV), num_atoms=nat_t.to(DEV),
                          node2graph=torch.arange(B).repeat_interleave(nat_t).to(DEV), t=te,
                          text_embeds=cn[0].expand(B, -1).to(DEV))
        outs.append([o.node_features.cpu(), o.atom_types_out.cpu(), o.coords_out.cpu(), o.lattice_out.cpu()])
        took.append([lib.chm_batch_short_row_tiles(b.handle) for b in model.decoder._batches.values()])
    del model
    torch.cuda.empty_cache()
    assert took[0] == [-1] and took[1] == [0], took
    for u, v, what in zip(outs[0], outs[1], ("nodes", "types", "coords", "lattice")):
        assert torch.equal(u, v), f"{what}: the mixed row tiling differs from the uniform one"
