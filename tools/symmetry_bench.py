#!/usr/bin/env python
"""Cost of finding the crystal systems (with the atoms) of a final state on the device.

    python tools/symmetry_bench.py                  # 512x40, 64x20 and the worst case, each in a fresh child
    python tools/symmetry_bench.py --shape 64x20    # one shape in this process
    python tools/symmetry_bench.py --shape worst    # one crystal of 256 atoms: a 4x8x8 simple-cubic cell

Per shape one JSON line. For SAMPLESxATOMS the state is the final state of a T = 100 run (noise="philox",
synthetic weights); "worst" is the slowest legal input, 16 operations x 256 translations that are all accepted.
  device_ms          symmetry_states end to end: the cell pass, the symmetry pass, the records' copy to the host,
                     unpacking (median of --repeats)
  cell_kernel_ms     k_cell alone, between two device events (median of --repeats)
  kernel_ms          k_symm alone, between two device events (median of --repeats)
and the systems found, the largest n_sym and the number of flagged records. Nothing is compared here: the checks
against the restatements are tests/test_gpu_symmetry.py.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ("512x40", "64x20", "worst")


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", help="SAMPLESxATOMS or worst; default: every shape of %s, one child process each" % (SHAPES,))
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    p.add_argument("--out", help="append the JSON lines to this file as well")
    return p.parse_args()


def final_state(args, dev):
    import torch

    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds

    if args.shape == "worst":
        import numpy as np
        frac = np.array([[i / 4, j / 8, k / 8] for i in range(4) for j in range(8) for k in range(8)], dtype=np.float32)
        lat = np.diag([12.0, 24.0, 24.0]).astype(np.float32)[None]
        return [256], torch.full((256,), 29, dtype=torch.long, device=dev), torch.from_numpy(frac).to(dev), \
            torch.from_numpy(lat).to(dev), 0
    n_samples, n_atoms = (int(v) for v in args.shape.split("x"))
    natoms = [n_atoms] * n_samples
    cfg = default_config()
    cfg["timesteps"] = 100
    torch.manual_seed(0)
    model = Chemeleon(cfg)
    model.decoder.load_state_dict(synthetic_state_dict(default_config()))
    model = model.to(dev).eval()
    cond, null = synthetic_text_embeds(512)
    last = None
    for last in model.sample_states(natoms, None, 2.0, 1e-5, clone=False, noise="philox", seed=args.seed,
                                    text_embeds=cond.to(dev), null_text_embeds=null.to(dev)):
        pass
    _, a, x, lat = last
    return natoms, a.clone(), x.clone(), lat.clone(), model.num_timesteps


def run_shape(args):
    import numpy as np
    import torch

    from chemeleon_amd import Symmetry, symmetry_states
    from chemeleon_amd import cell as cell_module
    from chemeleon_amd.symmetry import RECORD_BYTES, symmetry_plan

    if not torch.cuda.is_available():
        raise SystemExit("symmetry_bench.py: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    natoms, a, x, lat, T = final_state(args, dev)
    sym = Symmetry()
    rep = symmetry_states(natoms, a, x, lat, sym)  # (plans, allocations and code load once before anything is timed)
    torch.cuda.synchronize()

    device_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rep = symmetry_states(natoms, a, x, lat, sym)
        device_ms.append((time.perf_counter() - t0) * 1e3)
    cells, plan = cell_module.cell_plan(natoms, dev), symmetry_plan(natoms, dev)
    cell_rec = torch.empty(len(natoms) * cell_module.RECORD_BYTES, dtype=torch.uint8, device=dev)
    out = torch.empty(len(natoms) * RECORD_BYTES, dtype=torch.uint8, device=dev)
    cell_ms, kernel_ms = [], []
    for _ in range(args.repeats):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        cells.run(lat, None, sym.symprec, sym.angle_tolerance, cell_rec)
        e1.record()
        plan.run(cell_rec, a, x, lat, None, sym.symprec, sym.angle_tolerance, out)
        e2.record()
        e2.synchronize()
        cell_ms.append(e0.elapsed_time(e1))
        kernel_ms.append(e1.elapsed_time(e2))
    names, found = np.unique(rep.system, return_counts=True)
    return {
        "bench": "symmetry", "shape": args.shape, "T": T, "noise": "philox", "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0), "device_ms": round(statistics.median(device_ms), 4),
        "cell_kernel_ms": round(statistics.median(cell_ms), 4), "kernel_ms": round(statistics.median(kernel_ms), 4),
        "records": len(natoms), "systems": {str(n) or "none": int(c) for n, c in zip(names, found)},
        "n_sym_max": int(rep.n_sym.max()), "n_pivot_max": int(rep.n_pivot.max()), "halvings_max": int(rep.halvings.max()),
        "flagged": int((rep.flags != 0).sum()),
    }


def emit(line, out):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    args = parse()
    if args.shape:
        emit(json.dumps(run_shape(args)), args.out)
        return 0
    for shape in SHAPES:  # a fresh process per shape, each under its own limit; nothing more after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--repeats", str(args.repeats), "--seed",
               str(args.seed)]
        if args.out:
            cmd += ["--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"symmetry_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"symmetry_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
