"""Streaming output on the device: k_state_snapshot against the host path (schema.step_to_atoms), for crystals of
up to 130 atoms and for crystals around and above the 1024 sort keys the kernel stages at a time, the
argument checks and graph capture of chm_snapshot_run, and the overlapped generator
(_sample_generator(overlap=True) over schema.StateStreamer) against the blocking one, step by step and
exactly."""

import ctypes

import numpy as np
import pytest
import torch

from chemeleon_amd import _lib
from chemeleon_amd.config import default_config
from chemeleon_amd.modules import schema
from chemeleon_amd.modules.schema import slot_layout, slot_to_atoms, step_to_atoms, symbol_rank_table
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

DEV = "cuda"
NATOMS = [1, 2, 63, 64, 65, 130, 7]  # one atom, around the wave width, two and three passes of the wave
POOL = [0, 1, 2, 6, 17, 20, 103, 104, 500]  # X, H, He, C, Cl, Ca, Lr and two classes the clamp sends to X
# above the 1024 keys the kernel stages at a time: one key short of a chunk, a full chunk, one more (two stagings per
# 64 atoms), a small crystal between them, and three stagings with a tail that is no multiple of 4 or 64
NATOMS_BIG = [1023, 1024, 1025, 3, 2113]
NEGATIVE = -7  # a class the sampler never produces: the kernel clamps it to X, step_to_atoms refuses it


def same_structures(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g.numbers), np.asarray(w.numbers))
        assert list(g.get_chemical_symbols()) == list(w.get_chemical_symbols())
        np.testing.assert_array_equal(np.asarray(g.cell), np.asarray(w.cell))
        np.testing.assert_array_equal(g.get_scaled_positions(), w.get_scaled_positions())


class Plan:
    def __init__(self, natoms):
        self.natoms = list(natoms)
        nat = (ctypes.c_int32 * len(natoms))(*natoms)
        rank = symbol_rank_table()
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().chm_snapshot_create(nat, len(natoms), rank.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                   104, ctypes.byref(self.handle)), "chm_snapshot_create")
        self.slot_bytes = int(_lib.load().chm_snapshot_slot_bytes(self.handle))

    def run(self, a, x, lat, slot, n_a=None, n_x=None, n_l=None, n_s=None):
        return _lib.load().chm_snapshot_run(
            self.handle, _lib.ptr(a), a.numel() if n_a is None else n_a, _lib.ptr(x),
            x.numel() if n_x is None else n_x, _lib.ptr(lat), lat.numel() if n_l is None else n_l, _lib.ptr(slot),
            slot.numel() if n_s is None else n_s, _lib.stream_handle())

    def close(self):
        _lib.load().chm_snapshot_destroy(self.handle)


def seeded_state(natoms, seed):
    N, B = sum(natoms), len(natoms)
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor(POOL)
    a = pool[torch.randint(0, len(pool), (N,), generator=g)]
    off = sum(natoms[:4])
    a[off:off + natoms[4]] = 20  # one crystal (65 atoms) of a single element
    return a, torch.rand(N, 3, generator=g), torch.randn(B, 3, 3, generator=g)


def seeded_state_big(seed):
    """NATOMS_BIG: the pool and the negative class, and in every crystal that has them atoms 1000 to 1100 (or to its
    end) of one element, so that equal symbols lie on both sides of a chunk boundary."""
    N, B = sum(NATOMS_BIG), len(NATOMS_BIG)
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor(POOL + [NEGATIVE])
    a = pool[torch.randint(0, len(pool), (N,), generator=g)]
    off = 0
    for n, element in zip(NATOMS_BIG, (17, 6, 17, 0, 6)):
        if n > 1000:
            a[off + 1000:off + min(n, 1100)] = element
        off += n
    assert (a == NEGATIVE).sum() > 100
    return a, torch.rand(N, 3, generator=g), torch.randn(B, 3, 3, generator=g)


@pytest.fixture(scope="module")
def plan():
    p = Plan(NATOMS)
    yield p
    p.close()


@pytest.fixture(scope="module")
def big_plan():
    p = Plan(NATOMS_BIG)
    yield p
    p.close()


@pytest.mark.parametrize("which", ["to_130_atoms", "above_1024_atoms"])
def test_kernel_matches_step_to_atoms(request, which):
    big = which == "above_1024_atoms"
    plan = request.getfixturevalue("big_plan" if big else "plan")
    NATOMS = plan.natoms
    a, x, lat = seeded_state_big(11) if big else seeded_state(NATOMS, 11)
    assert plan.slot_bytes == slot_layout(NATOMS)["bytes"]
    slot = torch.zeros(plan.slot_bytes, dtype=torch.uint8, device=DEV)
    ad, xd, ld = a.to(DEV), x.to(DEV), lat.to(DEV)
    assert plan.run(ad, xd, ld, slot) == 0, _lib.load().chm_last_error()
    host = slot.cpu().numpy()
    # (step_to_atoms gets the negative class as the X the kernel clamps it to: it refuses a negative number)
    same_structures(slot_to_atoms(host, NATOMS), step_to_atoms(torch.where(a < 0, 0, a), x, lat, NATOMS))
    # perm: per crystal a permutation that maps the sorted rows to their sources, equal symbols in source order
    lay, N = slot_layout(NATOMS), sum(NATOMS)
    perm = host[lay["perm"]:lay["numbers"]].view(np.int32)
    num = host[lay["numbers"]:lay["numbers"] + N]
    sx = host[lay["frac"]:lay["perm"]].view(np.float32).reshape(N, 3)
    clamped = torch.where((a >= 0) & (a <= 103), a, 0).numpy()
    off = 0
    for n in NATOMS:
        p = perm[off:off + n]
        assert sorted(p.tolist()) == list(range(n))
        np.testing.assert_array_equal(num[off:off + n], clamped[off:off + n][p])
        np.testing.assert_array_equal(sx[off:off + n], x.numpy()[off:off + n][p])
        same = num[off + 1:off + n] == num[off:off + n - 1]
        assert np.all(p[1:][same] > p[:-1][same])
        if n > 1025:  # the forced run comes out in source order, across the boundary between two stagings
            run = p[np.isin(p, np.arange(1000, 1100))]
            assert run.tolist() == list(range(1000, 1100)) and len(set(clamped[off + 1000:off + 1100])) == 1
        off += n


def test_run_refuses_mis_sized_buffers(plan):
    a, x, lat = (t.to(DEV) for t in seeded_state(NATOMS, 12))
    slot = torch.full((plan.slot_bytes,), 0xAB, dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    N, B = sum(NATOMS), len(NATOMS)
    for kw, name in [({"n_a": N - 1}, b"atom_types"), ({"n_x": 3 * N + 3}, b"frac"), ({"n_l": 9 * B - 9}, b"lattices"),
                     ({"n_s": plan.slot_bytes - 16}, b"slot"), ({"n_s": plan.slot_bytes + 16}, b"slot")]:
        assert plan.run(a, x, lat, slot, **kw) == -1, kw
        assert name in lib.chm_last_error(), (kw, lib.chm_last_error())
    torch.cuda.synchronize()
    assert bool((slot == 0xAB).all())  # nothing was enqueued
    assert plan.run(a, x, lat, slot) == 0
    torch.cuda.synchronize()


def test_run_under_graph_capture(plan):
    a0, x0, l0 = seeded_state(NATOMS, 13)
    a1, x1, l1 = seeded_state(NATOMS, 14)
    a, x, lat = a0.to(DEV), x0.to(DEV), l0.to(DEV)
    slot = torch.zeros(plan.slot_bytes, dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert plan.run(a, x, lat, slot) == 0
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    first = slot.cpu().numpy().copy()
    a.copy_(a1), x.copy_(x1), lat.copy_(l1)
    g.replay()
    second = slot.cpu().numpy().copy()
    same_structures(slot_to_atoms(first, NATOMS), step_to_atoms(a0, x0, l0, NATOMS))
    same_structures(slot_to_atoms(second, NATOMS), step_to_atoms(a1, x1, l1, NATOMS))


# --------------------------------------------------------------------------- the streaming generator
@pytest.fixture(scope="module")
def model100():
    from chemeleon_amd import Chemeleon
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    m = Chemeleon(cfg)
    m.decoder.load_state_dict(synthetic_state_dict(default_config()))
    return m.to(DEV).eval()


def stream_run(model, noise, t_stop, overlap):
    cond, null = synthetic_text_embeds(512)
    torch.manual_seed(21)
    steps = list(model._sample_generator([3, 5, 8], None, 2.0, 1e-5, noise=noise, seed=4, text_embeds=cond,
                                         null_text_embeds=null, t_stop=t_stop, overlap=overlap))
    return steps, torch.get_rng_state()


@pytest.mark.parametrize("noise", ["torch", "philox"])
def test_overlapped_stream_equals_blocking(model100, noise):
    blocking, rng_b = stream_run(model100, noise, 90, False)
    overlapped, rng_o = stream_run(model100, noise, 90, True)
    assert len(blocking) == len(overlapped) == 10
    for got, want in zip(overlapped, blocking):
        same_structures(got, want)
    assert torch.equal(rng_b, rng_o)  # (noise="torch": the exhausted generator leaves the CPU stream where it was)


def test_ring_reuse_keeps_earlier_structures(model100, monkeypatch):
    """20 steps through a 2-slot ring: every slot is written 10 times, and every step's structures are
    compared only at the end, so a structure that still pointed into its (reused) slot would show."""
    made = []

    class Recording(schema.StateStreamer):
        def __init__(self, natoms, device, slots=2):
            super().__init__(natoms, device, slots=2)
            made.append(self)

    blocking, _ = stream_run(model100, "philox", 80, False)
    monkeypatch.setattr(schema, "StateStreamer", Recording)
    overlapped, _ = stream_run(model100, "philox", 80, True)
    assert len(made) == 1 and len(made[0].uses) == 2 and min(made[0].uses) >= 5, made[0].uses
    assert len(blocking) == len(overlapped) == 20
    for got, want in zip(overlapped, blocking):
        same_structures(got, want)
