#!/usr/bin/env python
"""Streaming-output cost: ms per reverse step of the plain state loop against the two structure generators.

    python tools/stream_bench.py                  # 512x40 and 64x20, each in a fresh child under a time limit
    python tools/stream_bench.py --shape 64x20    # one shape in this process

Per shape one JSON line: ms per step of
  plain     sample_states (device states, no conversion),
  blocking  _sample_generator(overlap=False) (step_to_atoms per step),
  overlap   _sample_generator(overlap=True)  (device snapshot + conversion one step behind),
the two ratios to the plain loop of the same run, and the host time of one conversion by either path (what a
ratio above 1 has to hide or pay). T = 1000 schedule, noise="philox", synthetic weights, `--steps` timed steps
after `--warmup`; a window is timed with the host clock between two device synchronisations. The three modes
alternate `--repeats` times in one process and the median window counts (all windows are in the line).
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
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    p.add_argument("--out", help="append the JSON lines to this file as well")
    return p.parse_args()


def run_shape(args):
    import torch

    from chemeleon_amd import Chemeleon
    from chemeleon_amd.config import default_config
    from chemeleon_amd.modules.schema import StateStreamer, step_to_atoms
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds

    if not torch.cuda.is_available():
        raise SystemExit("stream_bench.py: needs a HIP device (nothing is measured without one)")
    n_samples, n_atoms = (int(v) for v in args.shape.split("x"))
    natoms = [n_atoms] * n_samples
    dev = torch.device("cuda", 0)
    cfg = default_config()
    torch.manual_seed(0)
    model = Chemeleon(cfg)
    model.decoder.load_state_dict(synthetic_state_dict(cfg))
    model = model.to(dev).eval()
    cond, null = synthetic_text_embeds(512)
    kw = dict(noise="philox", seed=args.seed, text_embeds=cond.to(dev), null_text_embeds=null.to(dev))

    def window(mode):
        if mode == "plain":
            it = model.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw)
            next(it)  # the initial state
        else:
            it = model._sample_generator(natoms, None, 2.0, 1e-5, overlap=(mode == "overlap"), **kw)
        for _ in range(args.warmup):
            next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            next(it)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        it.close()
        torch.cuda.synchronize()
        return ms

    modes = ("plain", "blocking", "overlap")
    for m in modes:  # every mode's code paths, allocations and graph capture once before anything is timed
        window(m)
    runs = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:
            runs[m].append(window(m))
    med = {m: statistics.median(v) for m, v in runs.items()}

    # host time of one conversion, device idle: what each generator spends on the host per step
    it = model.sample_states(natoms, None, 2.0, 1e-5, clone=False, **kw)
    next(it)
    _, a, x, lat = next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        step_to_atoms(a, x, lat, natoms)
    host_blocking = (time.perf_counter() - t0) / 10 * 1e3
    st = StateStreamer(natoms, dev)
    st.pop(st.push(a, x, lat))
    t0 = time.perf_counter()
    for _ in range(10):
        st.pop(st.push(a, x, lat))
    host_overlap = (time.perf_counter() - t0) / 10 * 1e3
    st.close()
    it.close()
    return {
        "bench": "stream", "shape": args.shape, "T": model.num_timesteps, "noise": "philox", "steps": args.steps,
        "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
        "ms_per_step_plain": round(med["plain"], 4), "ms_per_step_blocking": round(med["blocking"], 4),
        "ms_per_step_overlap": round(med["overlap"], 4),
        "ratio_blocking": round(med["blocking"] / med["plain"], 4),
        "ratio_overlap": round(med["overlap"] / med["plain"], 4),
        "windows_ms": {m: [round(v, 4) for v in runs[m]] for m in modes},
        "host_ms_step_to_atoms": round(host_blocking, 4),
        "host_ms_snapshot_copy_slot_to_atoms": round(host_overlap, 4),
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
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--repeats", str(args.repeats), "--seed", str(args.seed)]
        if args.out:
            cmd += ["--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"stream_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"stream_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
