#!/usr/bin/env python
"""Cost of reducing a final state to primitive cells on the device.

    python tools/primitive_bench.py                  # 512x40, 64x20 and the worst case, each in a fresh child
    python tools/primitive_bench.py --shape 64x20    # one shape in this process
    python tools/primitive_bench.py --shape worst    # one crystal of 256 atoms: a 4x8x8 simple-cubic cell

Per shape one JSON line. For SAMPLESxATOMS the state is the final state of a T = 100 run (noise="philox",
synthetic weights); "worst" is the slowest legal input, 256 translations of one species that are all accepted.
  device_ms          primitive_states end to end: the cell pass, the primitive pass, the records' copy to the
                     host, unpacking (median of --repeats)
  cell_kernel_ms     k_cell alone, between two device events (median of --repeats)
  kernel_ms          k_prim_clear, k_prim, k_prim_offsets and k_prim_pack together, between two device events
                     (median of --repeats)
and the atoms before and after, the largest m and the number of flagged records. Nothing is compared here: the
checks against the restatements are tests/test_gpu_primitive.py.
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
    import torch

    from chemeleon_amd import Primitive, primitive_states
    from chemeleon_amd import cell as cell_module
    from chemeleon_amd.primitive import RECORD_BYTES, primitive_plan

    if not torch.cuda.is_available():
        raise SystemExit("primitive_bench.py: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    natoms, a, x, lat, T = final_state(args, dev)
    prim = Primitive()
    rep = primitive_states(natoms, a, x, lat, prim)[4]  # (plans, allocations and code load once before anything is timed)
    torch.cuda.synchronize()

    device_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rep = primitive_states(natoms, a, x, lat, prim)[4]
        device_ms.append((time.perf_counter() - t0) * 1e3)
    B, N = len(natoms), sum(natoms)
    cells, plan = cell_module.cell_plan(natoms, dev), primitive_plan(natoms, dev)
    cell_rec = torch.empty(B * cell_module.RECORD_BYTES, dtype=torch.uint8, device=dev)
    out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
    source = torch.empty(N, dtype=torch.int32, device=dev)
    new_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    a_p, x_p, lat_p = torch.empty_like(a), torch.empty_like(x), torch.empty_like(lat)
    cell_ms, kernel_ms = [], []
    for _ in range(args.repeats):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        cells.run(lat, None, prim.symprec, prim.angle_tolerance, cell_rec)
        e1.record()
        plan.run(cell_rec, a, x, lat, prim.symprec, prim.angle_tolerance, out, source, new_off, a_p, x_p, lat_p)
        e2.record()
        e2.synchronize()
        cell_ms.append(e0.elapsed_time(e1))
        kernel_ms.append(e1.elapsed_time(e2))
    return {
        "bench": "primitive", "shape": args.shape, "T": T, "noise": "philox", "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0), "device_ms": round(statistics.median(device_ms), 4),
        "cell_kernel_ms": round(statistics.median(cell_ms), 4), "kernel_ms": round(statistics.median(kernel_ms), 4),
        "records": B, "atoms": N, "atoms_after": int(rep.n_prim.sum()), "reduced": int(rep.reduced.sum()),
        "n_trans_max": int(rep.n_trans.max()), "n_pivot_max": int(rep.n_pivot.max()),
        "halvings_max": int(rep.halvings.max()), "flagged": int((rep.flags != 0).sum()),
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
            print(f"primitive_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"primitive_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
