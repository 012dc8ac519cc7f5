"""bench.py's plain run and `--dump-outputs`: one small run of the script (8 crystals of 6 atoms, 1 warm-up
and 2 timed steps), started once for the module. The result line holds the headline and none of the
`--full` legs, and the dumped arrays are the state the timed path reached: the same sampling path iterated
here, from the same seeded inputs, over the same 3 reverse steps.
Run on an MI355X: pytest -m gpu."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, NA, WARMUP, STEPS = 8, 6, 1, 2


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bench") / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--n-samples", str(B), "--n-atoms", str(NA), "--dump-outputs", d],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), d


def test_plain_result_line(run):
    line, _ = run
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["unit"] == "structures/sec" and line["higher_is_better"] is True
    assert abs(line["value"] - B / line["ms_per_step"]) < 1e-9 * line["value"]  # B / (T * s_per_step), T = 1000
    for k in ("roofline", "msgpass", "edge_layer1", "edge_layer2", "api", "cpu_baseline", "edge_events"):
        assert k not in line, f"{k} belongs to --full"


def test_dumped_outputs_are_the_timed_path_state(run):
    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
    _, d = run
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in ("atom_types", "frac_coords", "lattices")}
    assert sorted(os.listdir(d)) == ["atom_types.npy", "frac_coords.npy", "lattices.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["atom_types"].shape == (B * NA,) and got["frac_coords"].shape == (B * NA, 3)
    assert got["lattices"].shape == (B, 3, 3)
    # the benchmark's inputs: weights and conditioning of the synthetic recipe, initial noise of seed 0
    cfg = default_config()
    torch.manual_seed(0)
    model = Chemeleon(cfg)
    model.decoder.load_state_dict(synthetic_state_dict(cfg))
    model = model.to("cuda:0").eval()
    model.decoder.set_math("split16")
    cond, null = synthetic_text_embeds(512)
    gen = torch.Generator().manual_seed(0)
    l_init = torch.randn(B, 3, 3, generator=gen) * torch.tensor([[1, 0, 1], [1, 1, 1], [0, 0, 1]]).bool()
    x_init = torch.randn(B * NA, 3, generator=gen)
    it = model.sample_states([NA] * B, None, 2.0, 1e-5, noise="philox", seed=0, text_embeds=cond.to("cuda:0"),
                             null_text_embeds=null.to("cuda:0"), clone=False, init=(l_init, x_init))
    for _ in range(1 + WARMUP + STEPS):
        t, a, x, lat = next(it)
    it.close()
    assert t == 1000 - WARMUP - STEPS
    a, x, lat = a.cpu().numpy(), x.cpu().numpy(), lat.cpu().numpy()
    dx = np.abs(got["frac_coords"] - x)
    dx = np.minimum(dx, 1 - dx)  # (fractional coordinates wrap)
    dl = np.abs(got["lattices"] - lat).max()
    print(f"max |dx| {dx.max():.3e}, max |dl| {dl:.3e} (|l| max {np.abs(lat).max():.3e})")
    # the same kernels on the same inputs: at most fp32 rounding of a different summation order in three
    # steps, bounded as smoke() bounds one step against the CPU oracle
    assert np.array_equal(got["atom_types"], a.astype(np.float32))
    assert dx.max() < 1e-4
    assert dl <= 1e-4 * np.abs(lat).max()
