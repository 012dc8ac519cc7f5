#!/usr/bin/env python
"""Cost of classifying and reducing the cells of a final state: the device path against the plain host path.

    python tools/cell_bench.py                  # 512x40 and 64x20, each in a fresh child under a time limit
    python tools/cell_bench.py --shape 64x20    # one shape in this process

Per shape one JSON line, for the final state of a T = 100 run (noise="philox", synthetic weights):
  device_ms          cell_states end to end: launch, the records' copy to the host, unpacking (median of --repeats)
  reduce_ms          reduce_states end to end: both launches and the records' copy (median of --repeats)
  kernel_ms          k_cell alone, between two device events (median of --repeats)
  apply_ms           k_cell_apply alone, between two device events (median of --repeats)
  host_ms            the plain host path: the lattices' copy to the host plus the numpy float64 restatement of
                     tests/cell_cases.py (reduction, search, table, halving) per crystal (one run)
  host_copy_ms       the copy's share of host_ms
and how many records agree with that restatement (system, counts, halvings and flags equal), the smallest margin
of the restatement's decisions (below 1e-3 a float32 search may legitimately decide a candidate differently), and
the systems found.
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

SHAPES = ("512x40", "64x20")


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", help="SAMPLESxATOMS; default: every shape of %s, one child process each" % (SHAPES,))
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    p.add_argument("--out", help="append the JSON lines to this file as well")
    return p.parse_args()


def run_shape(args):
    import numpy as np
    import torch

    from chemeleon_amd import Cell, Chemeleon, cell_states, reduce_states
    from chemeleon_amd.cell import RECORD_BYTES, cell_plan
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
    from tests import cell_cases as C

    if not torch.cuda.is_available():
        raise SystemExit("cell_bench.py: needs a HIP device (nothing is measured without one)")
    n_samples, n_atoms = (int(v) for v in args.shape.split("x"))
    natoms = [n_atoms] * n_samples
    dev = torch.device("cuda", 0)
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
    a, x, lat = a.clone(), x.clone(), lat.clone()
    cell = Cell()
    rep = cell_states(natoms, a, x, lat, cell)  # (plan, allocations and code load once before anything is timed)
    reduce_states(natoms, a, x, lat, cell)
    torch.cuda.synchronize()

    device_ms, reduce_ms = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rep = cell_states(natoms, a, x, lat, cell)
        device_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        reduce_states(natoms, a, x, lat, cell)
        reduce_ms.append((time.perf_counter() - t0) * 1e3)
    plan = cell_plan(natoms, dev)
    out = torch.empty(len(natoms) * RECORD_BYTES, dtype=torch.uint8, device=dev)
    xo, lo = torch.empty_like(x), torch.empty_like(lat)
    kernel_ms, apply_ms = [], []
    for _ in range(args.repeats):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        plan.run(lat, None, cell.symprec, cell.angle_tolerance, out)
        e1.record()
        plan.apply(out, x, lat, xo, lo)
        e2.record()
        e2.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
        apply_ms.append(e1.elapsed_time(e2))

    t0 = time.perf_counter()
    lh = lat.cpu().numpy()
    t1 = time.perf_counter()
    ref = [C.classify(lh[g], cell.symprec, cell.angle_tolerance) for g in range(len(natoms))]
    t2 = time.perf_counter()
    decided = C.DEGENERATE | C.NONFINITE | C.AMBIGUOUS | C.MISMATCH | C.NOT_REDUCED
    agree = [r["code"] == rep.code[g] and r["counts"] == (int(rep.n_ops[g]),) + tuple(int(v) for v in rep.orders[g])
             and r["halvings"] == rep.halvings[g] and r["flags"] & decided == int(rep.flags[g]) & decided
             for g, r in enumerate(ref)]
    names, found = np.unique(rep.system, return_counts=True)
    return {
        "bench": "cell", "shape": args.shape, "T": model.num_timesteps, "noise": "philox", "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0), "device_ms": round(statistics.median(device_ms), 4),
        "reduce_ms": round(statistics.median(reduce_ms), 4), "kernel_ms": round(statistics.median(kernel_ms), 4),
        "apply_ms": round(statistics.median(apply_ms), 4), "host_ms": round((t2 - t0) * 1e3, 2),
        "host_copy_ms": round((t1 - t0) * 1e3, 4), "records_agree": int(sum(agree)), "records": len(natoms),
        "smallest_margin": round(min(r["margin"] for r in ref), 6),
        "systems": {str(n) or "none": int(c) for n, c in zip(names, found)},
        "halvings_max": int(rep.halvings.max()), "passes_max": int(rep.passes.max()),
        "transform_max": int(np.abs(rep.transform).max()),
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
            print(f"cell_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"cell_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
