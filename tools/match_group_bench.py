#!/usr/bin/env python
"""Cost of grouping a final state's duplicates by matching: the device path, the fingerprint Dedup on the same
state, and a host loop of match_states over the leaders.

    python tools/match_group_bench.py                  # 512x40 and 64x20, each in a fresh child under a time limit
    python tools/match_group_bench.py --shape 64x20    # one shape in this process

Per shape one JSON line, for the final state of a T = 100 run (noise="philox", synthetic weights):
  cell_ms            k_cell alone, between two device events (median of --repeats)
  group_ms           chm_match_group_run alone (the clear, k_match_pairs, k_dedup_lead, the gather), between two
                     device events (median of --repeats)
  device_ms          match_group_states end to end: the launches and the report's copy to the host (median)
  dedup_ms           dedup_states (the fingerprint Dedup, default tol) end to end on the same state (median)
  host_loop_ms       the leader rule as a host loop: one match_states call per leader, against that leader as a
                     Reference (one run), and how many calls it took
  pairs              pairs launched (all of equal atom count), and how many reached the mapping search / matched
  groups             groups found by the new path, by the host loop and by the fingerprint Dedup
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
    p.add_argument("--limit", type=int, default=400, help="seconds a shape's child process may take")
    p.add_argument("--out", help="append the JSON lines to this file as well")
    return p.parse_args()


def run_shape(args):
    import numpy as np
    import torch

    from chemeleon_amd import (Chemeleon, Dedup, Match, MatchDedup, Reference, dedup_states, match_group_states,
                               match_states)
    from chemeleon_amd import cell as cell_module
    from chemeleon_amd.config import default_config
    from chemeleon_amd.match_group import PAIR_RECORD_BYTES, RECORD_BYTES, match_group_plan
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds

    if not torch.cuda.is_available():
        raise SystemExit("match_group_bench.py: needs a HIP device (nothing is measured without one)")
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
    md, dd = MatchDedup(), Dedup()
    rep = match_group_states(natoms, a, x, lat, md)  # (plans, allocations and code load once before anything is timed)
    fp_rep = dedup_states(natoms, a, x, lat, dd)
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

    def wall(fn):
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    B = len(natoms)
    cells, plan = cell_module.cell_plan(natoms, dev), match_group_plan(natoms, dev)
    cell_rec = torch.empty(B * cell_module.RECORD_BYTES, dtype=torch.uint8, device=dev)
    group = torch.empty(2, B, dtype=torch.int32, device=dev)
    out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
    pair_rec = torch.empty(plan.num_pairs * PAIR_RECORD_BYTES, dtype=torch.uint8, device=dev)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    cell_ms = events(lambda: cells.run(lat, None, 0.1, 10.0, cell_rec))
    group_ms = events(lambda: plan.run(cell_rec, a, x, lat, None, md.ltol, md.stol, md.angle_tol, group[0], group[1],
                                       out, pair_rec, ws))
    device_ms = wall(lambda: match_group_states(natoms, a, x, lat, md))
    dedup_ms = wall(lambda: dedup_states(natoms, a, x, lat, dd))

    # the leader rule as a host loop over match_states: every crystal still without a group is the next leader
    t0 = time.perf_counter()
    ah, xh, lh = a.cpu().numpy(), x.cpu().numpy(), lat.cpu().numpy()
    hgroup, calls = np.full(B, -1, dtype=np.int64), 0
    usable = rep.group >= 0
    for g in range(B):
        if hgroup[g] >= 0 or not usable[g]:
            continue
        hgroup[g] = g
        rest = np.flatnonzero((hgroup < 0) & usable & (np.arange(B) > g))
        if not len(rest):
            continue
        s = slice(g * n_atoms, (g + 1) * n_atoms)
        ref = Reference.from_arrays([n_atoms], ah[s], xh[s], lh[g:g + 1])
        got = match_states(natoms, a, x, lat, Match(ref))
        calls += 1
        hgroup[rest[got.matched[rest]]] = g
    host_loop_ms = (time.perf_counter() - t0) * 1e3

    return {
        "bench": "match_group", "shape": args.shape, "T": model.num_timesteps, "noise": "philox", "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0), "ltol": md.ltol, "stol": md.stol, "angle_tol": md.angle_tol,
        "cell_ms": round(cell_ms, 4), "group_ms": round(group_ms, 4), "device_ms": round(device_ms, 4),
        "dedup_ms": round(dedup_ms, 4), "host_loop_ms": round(host_loop_ms, 2), "host_loop_calls": calls,
        "pairs": int(plan.num_pairs), "pairs_searched": rep.n_searched, "pairs_matched": int(rep.pair_matched.sum()),
        "pairs_many_mappings": int(((rep.pair_flags & 32) != 0).sum()), "groups": rep.n_groups,
        "groups_host_loop": int((hgroup == np.arange(B)).sum()),
        "groups_agree": bool(np.array_equal(np.where(usable, hgroup, -1), rep.group)),
        "groups_dedup": fp_rep.n_groups, "no_cell": int((~usable).sum()), "records": B,
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
            print(f"match_group_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"match_group_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
