#!/usr/bin/env python
"""Cost of searching a reference set for every structure of a final state: the device path against a host loop of
match_states calls, one per candidate reference (what there was before chm_match_set_*).

    python tools/match_set_bench.py                  # 512x40 and 64x20, each in a fresh child under a time limit
    python tools/match_set_bench.py --shape 64x20    # one shape in this process

The set is synthetic and built from the final state of a T = 100 run (noise="philox", synthetic weights) itself:
every 4th sample as a disguised copy (atoms permuted, origin shifted, cell scaled by 1.05), every 8th sample's cell
with its own types permuted among its atoms (the sample's composition, another structure: a candidate that should
not match), and --fillers structures (default 4096) drawn from the samples' cells with fresh atom types, a third
of them with one atom less and a third with one atom more (other sizes). Per shape one JSON line:
  cell_ms            k_cell over the samples alone, between two device events (median of --repeats)
  set_ms             chm_match_set_run alone (keys, offsets, pairs, gather), between two device events (median)
  device_ms          match_set_states end to end: the launches and the report's copy to the host (median)
  host_loop_ms       one match_states call per distinct candidate reference, each against the samples whose
                     candidate it is; measured over the first --host-calls of them and scaled to all
  host_loop_agrees   the host loop's matched / rms of those calls equal the device's pair records, and where the
                     loop ran over every candidate its known / ref equal the device's
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
    p.add_argument("--fillers", type=int, default=4096)
    p.add_argument("--host-calls", type=int, default=64, help="candidate references the host loop is measured over")
    p.add_argument("--limit", type=int, default=400, help="seconds a shape's child process may take")
    p.add_argument("--out", help="append the JSON lines to this file as well")
    return p.parse_args()


def synthetic_set(n_atoms, a, x, lat, fillers, seed):
    """(natoms, types, frac, lattices, copy_of): the set described above; copy_of[r] = the sample reference r is a
    disguised copy of, or -1."""
    import numpy as np
    rng = np.random.default_rng(seed)
    B = len(lat)
    a, x = a.reshape(B, n_atoms), x.reshape(B, n_atoms, 3)
    out, copy_of = [], []
    for g in range(0, B, 4):
        p = rng.permutation(n_atoms)
        out.append((a[g][p], np.mod(x[g][p] + rng.uniform(0, 1, 3), 1.0), 1.05 * lat[g]))
        copy_of.append(g)
    for g in range(1, B, 8):
        out.append((rng.permutation(a[g]), x[g], lat[g]))
        copy_of.append(-1)
    elements = np.unique(a)
    for k in range(fillers):
        g = int(rng.integers(B))
        n = n_atoms + (k % 3 == 1) - (k % 3 == 2 and n_atoms > 1)
        out.append((rng.choice(elements, size=n), rng.uniform(0, 1, (n, 3)), lat[g]))
        copy_of.append(-1)
    order = rng.permutation(len(out))
    out, copy_of = [out[k] for k in order], np.array(copy_of)[order]
    return ([len(s[0]) for s in out], np.concatenate([s[0] for s in out]).astype(np.int64),
            np.concatenate([s[1] for s in out]).astype(np.float32), np.stack([s[2] for s in out]).astype(np.float32), copy_of)


def run_shape(args):
    import numpy as np
    import torch

    from chemeleon_amd import Chemeleon, Match, MatchSet, Reference, ReferenceSet, match_set_states, match_states
    from chemeleon_amd import cell as cell_module
    from chemeleon_amd.config import default_config
    from chemeleon_amd.match_set import PAIR_RECORD_BYTES, RECORD_BYTES, match_set_plan
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds

    if not torch.cuda.is_available():
        raise SystemExit("match_set_bench.py: needs a HIP device (nothing is measured without one)")
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
    rnat, rtypes, rfrac, rlat, copy_of = synthetic_set(n_atoms, a.cpu().numpy(), x.cpu().numpy(), lat.cpu().numpy(),
                                                       args.fillers, args.seed)
    t0 = time.perf_counter()
    rs = ReferenceSet.from_arrays(rnat, rtypes, rfrac, rlat)
    sort_ms = (time.perf_counter() - t0) * 1e3
    ms_ = MatchSet(rs)
    t0 = time.perf_counter()
    rep = match_set_states(natoms, a, x, lat, ms_)  # (the set's upload, plans and code load once before the timing)
    first_ms = (time.perf_counter() - t0) * 1e3
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
    cells, plan = cell_module.cell_plan(natoms, dev), match_set_plan(natoms, rs, dev)
    ra, rx, rl, rrec = rs.on(dev)
    cell_rec = torch.empty(B * cell_module.RECORD_BYTES, dtype=torch.uint8, device=dev)
    out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
    pair_rec = torch.empty(plan.num_pairs_max * PAIR_RECORD_BYTES, dtype=torch.uint8, device=dev)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    cell_ms = events(lambda: cells.run(lat, None, 0.1, 10.0, cell_rec))
    set_ms = events(lambda: plan.run(cell_rec, a, x, lat, rrec, ra, rx, rl, None, ms_.ltol, ms_.stol, ms_.angle_tol, out,
                                     pair_rec, ws))
    device_ms = wall(lambda: match_set_states(natoms, a, x, lat, ms_))

    # the host loop: one match_states call per distinct candidate reference, against the samples whose candidate it is
    given = Reference.from_arrays(rnat, rtypes, rfrac, rlat)
    offs = np.concatenate([[0], np.cumsum(rnat)])
    cands = sorted(set(rep.pair_ref.tolist()))
    todo = cands[:args.host_calls]
    agree, best = True, {}
    t0 = time.perf_counter()
    for r in todo:
        s = slice(offs[r], offs[r + 1])
        ref = Reference.from_arrays([rnat[r]], given.atom_types[s], given.frac_coords[s], given.lattices[r:r + 1])
        at = np.flatnonzero(rep.pair_ref == r)
        of = np.full(B, -1)
        of[rep.pair_sample[at]] = 0
        got = match_states(natoms, a, x, lat, Match(ref, ref_of=of.tolist()))
        for k in at:
            g = int(rep.pair_sample[k])
            agree &= bool(got.matched[g]) == bool(rep.pair_matched[k]) and got.rms[g].tobytes() == rep.pair_rms[k].tobytes()
            if got.matched[g]:
                best[g] = min(best.get(g, (np.inf, -1)), (float(got.rms[g]), r))
    host_ms = (time.perf_counter() - t0) * 1e3
    if len(todo) == len(cands):
        known = np.array([g in best for g in range(B)])
        ref = np.array([best[g][1] if g in best else -1 for g in range(B)])
        agree &= bool(np.array_equal(known, rep.known) and np.array_equal(ref, rep.ref))
    copies = np.flatnonzero(copy_of >= 0)
    return {
        "bench": "match_set", "shape": args.shape, "T": model.num_timesteps, "noise": "philox", "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0), "ltol": ms_.ltol, "stol": ms_.stol, "angle_tol": ms_.angle_tol,
        "references": len(rs), "references_of_sample_size": int((np.array(rnat) == n_atoms).sum()),
        "pairs_max": plan.num_pairs_max, "pairs": int(rep.n_candidates.sum()), "pairs_matched": int(rep.pair_matched.sum()),
        "known": rep.n_known, "novel": rep.n_novel, "copies": len(copies),
        "copies_found": int(sum(rep.ref[copy_of[r]] == r for r in copies)),
        "sort_ms": round(sort_ms, 3), "first_call_ms": round(first_ms, 2), "cell_ms": round(cell_ms, 4),
        "set_ms": round(set_ms, 4), "device_ms": round(device_ms, 4), "host_loop_calls": len(todo),
        "candidate_references": len(cands), "host_loop_measured_ms": round(host_ms, 2),
        "host_loop_ms": round(host_ms * len(cands) / max(1, len(todo)), 2), "host_loop_agrees": bool(agree), "records": B,
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
               str(args.seed), "--fillers", str(args.fillers), "--host-calls", str(args.host_calls)]
        if args.out:
            cmd += ["--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"match_set_bench.py: {shape} exceeded {args.limit} s", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"match_set_bench.py: {shape} exited with {rc}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
