#!/usr/bin/env python
"""Cost of grouping a final state's duplicates: the device path against the plain host path.

    python tools/dedup_bench.py                  # 512x40 and 64x20, each in a fresh child under a time limit
    python tools/dedup_bench.py --shape 64x20    # one shape in this process

Per shape one JSON line, for the final state of a T = 100 run (noise="philox", synthetic weights):
  fingerprint_ms     k_fingerprint alone, between two device events (median of --repeats)
  group_ms           k_dedup_match + k_dedup_lead, between two device events (median of --repeats)
  device_ms          dedup_states end to end: both launches, the report's copy to the host (median of --repeats)
  host_ms            the plain host path: the state's copy to the host, the numpy float64 fingerprints of
                     tests/dedup_cases.py per crystal and the plain-Python match and leader rules (one run)
  groups             groups found at the default tol on the device, and by the host path
  distance_hist      pairwise distances |F_g - F_h| / max(|F_g|, |F_h|) between crystals of equal reduced
                     composition (float64 fingerprints), counted per edge of --edges: what the default tol cuts
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
EDGES = (0.0, 0.00625, 0.0125, 0.025, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", help="SAMPLESxATOMS; default: every shape of %s, one child process each" % (SHAPES,))
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--limit", type=int, default=400, help="seconds a shape's child process may take")
    p.add_argument("--out", help="append the JSON lines to this file as well")
    return p.parse_args()


def run_shape(args):
    import numpy as np
    import torch

    from chemeleon_amd import Chemeleon, Dedup, dedup_states, fingerprint_states
    from chemeleon_amd.config import default_config
    from chemeleon_amd.dedup import group_on_device
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds
    from tests import dedup_cases as C

    if not torch.cuda.is_available():
        raise SystemExit("dedup_bench.py: needs a HIP device (nothing is measured without one)")
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
    dd = Dedup()
    rep = dedup_states(natoms, a, x, lat, dd)  # (plan, allocations and code load once before anything is timed)
    torch.cuda.synchronize()

    def events(fn):
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    fingerprint_ms = events(lambda: fingerprint_states(natoms, a, x, lat, dd))
    fps = fingerprint_states(natoms, a, x, lat, dd)
    group_ms = events(lambda: group_on_device(fps, dd.tol))
    device_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rep = dedup_states(natoms, a, x, lat, dd)
        device_ms.append((time.perf_counter() - t0) * 1e3)

    t0 = time.perf_counter()
    ah, xh, lh = a.cpu().numpy(), x.cpu().numpy(), lat.cpu().numpy()
    t1 = time.perf_counter()
    off = np.concatenate([[0], np.cumsum(natoms)])
    F, counts, flags = [], [], []
    for g in range(len(natoms)):
        s = slice(int(off[g]), int(off[g + 1]))
        F.append(C.fingerprint_f64(lh[g], xh[s], ah[s]))
        counts.append(C.reduced_counts(ah[s]))
        flags.append(C.flags_of(lh[g], xh[s]))
    D = C.distance_matrix(np.stack(F))
    ok = np.array(flags) == 0
    hgroup, hcount = C.leader(C.match_matrix(D, counts, ok, dd.tol), ok)
    t2 = time.perf_counter()

    F_dev = fps.fp.cpu().numpy()
    errs = [C.rel_error(F_dev[g], F[g]) for g in range(len(natoms)) if ok[g] and np.linalg.norm(F[g]) > 0]
    same = [D[g, h] for g in range(len(natoms)) for h in range(g + 1, len(natoms))
            if ok[g] and ok[h] and np.array_equal(counts[g], counts[h])]
    hist = np.histogram(same, bins=list(EDGES) + [np.inf])[0].tolist() if same else [0] * len(EDGES)
    return {
        "bench": "dedup", "shape": args.shape, "T": model.num_timesteps, "noise": "philox", "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0), "tol": dd.tol, "fingerprint_ms": round(fingerprint_ms, 4),
        "group_ms": round(group_ms, 4), "device_ms": round(statistics.median(device_ms), 4),
        "host_ms": round((t2 - t0) * 1e3, 2), "host_copy_ms": round((t1 - t0) * 1e3, 4), "groups": rep.n_groups,
        "groups_host": int((hcount > 0).sum()), "groups_agree": bool(np.array_equal(rep.group, hgroup)),
        "flagged": int((rep.flags != 0).sum()), "compositions": len({tuple(c) for c in counts}),
        "same_composition_pairs": len(same), "distance_edges": list(EDGES), "distance_hist": hist,
        "distance_min": round(float(min(same)), 5) if same else None,
        "fingerprint_error_max": float(max(errs)) if errs else None, "records": len(natoms),
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
            print(f"dedup_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"dedup_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
