"""What matching the final state against one reference costs (chemeleon_amd.match), end to end and per kernel, at
512x40 and 64x20 after a T = 100 run with synthetic weights, against the host path (a copy of the state plus the
tests' float64 restatement, tests/match_cases.py), and the slowest legal input: one 256-atom single-species
simple-cubic cell against itself, where no candidate is pruned. Prints one JSON line.

    python tools/match_bench.py [--host-crystals 16]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chemeleon_amd import Chemeleon, Match, Reference, match_states  # noqa: E402
from chemeleon_amd import cell as cell_module  # noqa: E402
from chemeleon_amd import match as match_module  # noqa: E402
from chemeleon_amd.config import default_config  # noqa: E402
from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds  # noqa: E402
from tests import match_cases as M  # noqa: E402
from tests import symmetry_cases as sc  # noqa: E402

DEV = "cuda"


def median_ms(fn, repeats=5):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def kernel_ms(natoms, a, x, lat, match, repeats=5):
    """(cell kernel, match kernel) medians in ms, from events on one stream."""
    B = len(natoms)
    ra, rx, rlat, rrec = match.reference.on(DEV)
    cells = cell_module.cell_plan(natoms, DEV)
    plan = match_module.match_plan(natoms, match.reference.natoms, match.ref_of_for(B), DEV)
    rec = torch.empty(B * 128, dtype=torch.uint8, device=DEV)
    out = torch.empty(B * 64, dtype=torch.uint8, device=DEV)
    tc, tm = [], []
    for _ in range(repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        cells.run(lat, None, 0.1, 10.0, rec)
        e[1].record()
        plan.run(rec, a, x, lat, rrec, ra, rx, rlat, match.ltol, match.stol, match.angle_tol, out)
        e[2].record()
        torch.cuda.synchronize()
        tc.append(e[0].elapsed_time(e[1]))
        tm.append(e[1].elapsed_time(e[2]))
    return float(np.median(tc)), float(np.median(tm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-crystals", type=int, default=16, help="crystals the host path is timed on (then scaled)")
    args = ap.parse_args()
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    model = Chemeleon(cfg)
    model.decoder.load_state_dict(synthetic_state_dict(default_config()))
    model = model.to(DEV).eval()
    cond, null = synthetic_text_embeds(512)
    result = {"tool": "match_bench", "shapes": {}}
    for B, n in ((512, 40), (64, 20)):
        natoms = [n] * B
        kw = dict(noise="philox", seed=4, text_embeds=cond, null_text_embeds=null)
        for _ in model.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw):  # (warm: plans and graph)
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = None
        for last in model.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw):
            pass
        torch.cuda.synchronize()
        step_ms = 1e3 * (time.perf_counter() - t0) / cfg["timesteps"]
        _, a, x, lat = last
        a, x, lat = a.clone(), x.clone(), lat.clone()
        ref = Reference.from_arrays([n], a[:n].cpu().numpy(), x[:n].cpu().numpy(), lat[:1].cpu().numpy())
        match = Match(ref)
        report = match_states(natoms, a, x, lat, match)  # (warm: plans, the reference on the device)
        end_to_end = median_ms(lambda: match_states(natoms, a, x, lat, match))
        cell_ms, match_ms = kernel_ms(natoms, a, x, lat, match)
        # the host path on the first crystals: the copy, then the float64 restatement
        K = min(B, args.host_crystals)
        t0 = time.perf_counter()
        ha, hx, hl = a.cpu().numpy(), x.cpu().numpy(), lat.cpu().numpy()
        rs = dict(lattice=hl[0], types=ha[:n], frac=hx[:n])
        host = [M.restate(dict(lattice=hl[g], types=ha[g * n:(g + 1) * n], frac=hx[g * n:(g + 1) * n]), rs) for g in range(K)]
        host_ms = 1e3 * (time.perf_counter() - t0)
        gate = 1.2e-5
        agree = all(int(report.matched[g]) == h["matched"] and int(report.flags[g]) == h["flags"] and
                    int(report.n_mappings[g]) == h["n_mappings"] and abs(float(report.rms[g]) - h["rms"]) <= gate
                    for g, h in enumerate(host))
        result["shapes"][f"{B}x{n}"] = dict(
            reverse_step_ms=step_ms, end_to_end_ms=end_to_end, k_cell_ms=cell_ms, k_match_ms=match_ms,
            host_crystals=K, host_ms_for_those=host_ms, host_ms_scaled_to_batch=host_ms * B / K,
            records_agree_with_float64=bool(agree), n_matched=report.n_matched,
            largest_n_mappings=int(report.n_mappings.max()), flags=sorted(set(report.flags.tolist())))
    # the slowest legal input
    L, types, frac = sc._supercell_sc(3.0, (4, 8, 8))
    s = dict(lattice=L.astype(np.float32), types=types, frac=frac.astype(np.float32))
    ref = Reference.from_arrays(*M.packed([s]))
    nat, t_, f_, l_ = M.packed([s])
    a, x, lat = (torch.from_numpy(v).to(DEV) for v in (t_, f_, l_))
    report = match_states(nat, a, x, lat, Match(ref))
    cell_ms, match_ms = kernel_ms(nat, a, x, lat, Match(ref), repeats=3)
    result["slowest"] = dict(atoms=256, k_match_ms=match_ms, n_mappings=int(report.n_mappings[0]),
                             n_candidates=int(report.n_candidates[0]), n_survivors=int(report.n_survivors[0]),
                             matched=bool(report.matched[0]))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
