#!/usr/bin/env python
"""Cost of a constraint: ms per reverse step with every atom type held against the unconstrained step.

    python tools/constraint_bench.py --shape 512x40 [--out FILE]

One JSON line: ms per step of the two modes (captured graph, noise="philox", T = 1000 schedule, synthetic
weights), their ratio and each mode's window-to-window spread ((max - min) / median). The modes alternate
`--repeats` times in one process, after one untimed window each; a window is `--steps` replays after `--warmup`,
timed with the host clock between two device synchronisations; the median window counts. The constrained step adds
one launch of k_constrain (stage 1; stage 2 launches nothing when no coordinates are held).
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="512x40", help="SAMPLESxATOMS")
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", help="append the JSON line to this file as well")
    args = p.parse_args()

    import torch

    from chemeleon_amd import Chemeleon, Constraint
    from chemeleon_amd.config import default_config
    from chemeleon_amd.synthetic import synthetic_state_dict, synthetic_text_embeds

    if not torch.cuda.is_available():
        raise SystemExit("constraint_bench.py: needs a HIP device (nothing is measured without one)")
    n_samples, n_atoms = (int(v) for v in args.shape.split("x"))
    natoms = [n_atoms] * n_samples
    dev = torch.device("cuda", 0)
    cfg = default_config()
    torch.manual_seed(0)
    model = Chemeleon(cfg)
    model.decoder.load_state_dict(synthetic_state_dict(cfg))
    model = model.to(dev).eval()
    cond, null = synthetic_text_embeds(512)
    kw = dict(noise="philox", seed=0, text_embeds=cond.to(dev), null_text_embeds=null.to(dev), clone=False)
    g = torch.Generator().manual_seed(1)
    numbers = torch.randint(1, 104, (n_samples, n_atoms), generator=g).tolist()
    con = Constraint.composition(natoms, numbers)

    def window(mode):
        it = model.sample_states(natoms, None, 2.0, 1e-5, constraint=con if mode == "constrained" else None, **kw)
        next(it)
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

    modes = ("free", "constrained")
    for m in modes:
        window(m)
    runs = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:
            runs[m].append(window(m))
    med = {m: statistics.median(v) for m, v in runs.items()}
    spread = {m: (max(v) - min(v)) / med[m] for m, v in runs.items()}
    line = json.dumps({
        "bench": "constraint", "shape": args.shape, "T": model.num_timesteps, "steps": args.steps,
        "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
        "ms_per_step_free": round(med["free"], 4), "ms_per_step_constrained": round(med["constrained"], 4),
        "ratio": round(med["constrained"] / med["free"], 5),
        "spread_free": round(spread["free"], 5), "spread_constrained": round(spread["constrained"], 5),
        "windows_ms": {m: [round(v, 4) for v in runs[m]] for m in modes}})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
