"""
BFS: the pooled search (`BFS.search_batch(..., slots=S)`, S games advancing together on the device) against the serial form (one
`search` after the other: `search_batch` without `slots`), on one MI355X, at the evaluation protocol's shape: 2 500 games, 500 each
of scrambling depths 1-5, under max_states 2 000, 20 000 and 175 000.  Both forms run the same games in one process; after a
warm-up run of each they alternate, and medians with min-max are shown; a pooled search takes milliseconds, so each of its
timings is a window of `--window` seconds of searches one after the other, divided by their number.  The pooled form runs at
several (S, C, K): slots, parents per slot and step, steps per round.  Every pooled run is compared with the serial one game by
game (solved, length, states).

    python tools/bfs_batch_probe.py --out profiles/bfs_batch_probe.json      (writes the .txt beside it)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd")]

DEPTHS = (1, 2, 3, 4, 5)


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": round(float(np.median(xs)), 6), "min": round(xs[0], 6), "max": round(xs[-1], 6)}


def scrambles(per_depth, seed):
    from librubiks import cube
    np.random.seed(seed)
    return np.concatenate([cube.scramble_batch(per_depth, d, True)[0].numpy() for d in DEPTHS])


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bfs_batch_probe.json")
    ap.add_argument("--per-depth", type=int, default=500)
    ap.add_argument("--caps", default="2000,20000,175000")
    ap.add_argument("--configs", default="2500:64:2,2500:256:1,2500:256:2,2500:256:4,2500:1024:2,2500:1024:4,256:256:4", help="S:C:K,...")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back searches per timing of a pooled form")
    args = ap.parse_args()
    from librubiks.solving.agents import BFS
    from librubiks.solving.bfs_batch_device import bfs_batch_plan
    states = scrambles(args.per_depth, 1)
    configs = [tuple(int(x) for x in c.split(":")) for c in args.configs.split(",")]
    out = {"games": len(states), "depths": list(DEPTHS), "caps": {}, "args": {k: v for k, v in vars(args).items() if k != "out"},
           "device": torch.cuda.get_device_name(0)}
    lines = [f"BFS pooled (slots=S, chunk C, K steps per round) against serial search_batch: {len(states)} games, {args.per_depth} each of "
             f"depths 1-5, {args.reps} alternated repetitions after a warm-up (median [min-max] milliseconds for all games; a pooled "
             f"timing is a window of >= {args.window} s of searches one after the other, divided by their number); {out['device']}"]
    for cap in (int(c) for c in args.caps.split(",")):
        serial = BFS()
        agents = {cfg: BFS(chunk=cfg[1], steps_per_round=cfg[2]) for cfg in configs}
        secs = {"serial": []}
        secs.update({cfg: [] for cfg in configs})
        same, calls = {}, {}

        def pooled(cfg, n):
            """n whole searches one after the other: a timed window of a pooled form is `--window` seconds of them, not one of a
            few milliseconds."""
            for _ in range(n):
                res = agents[cfg].search_batch(states, None, cap, slots=cfg[0])
            return res
        for rep in range(args.reps + 1):                  # rep 0: warm-up of every form
            dt, ref = timed(lambda: serial.search_batch(states, None, cap))
            if rep:
                secs["serial"].append(dt)
            for cfg in configs:                           # the forms alternate: serial, then every pooled shape, and again
                if not rep:
                    pooled(cfg, 1)                        # (allocates the batch, which then stays, as the serial form's does)
                    calls[cfg] = int(min(500, max(1, np.ceil(args.window / timed(lambda: pooled(cfg, 1))[0]))))
                dt, res = timed(lambda: pooled(cfg, calls[cfg]))
                same[cfg] = bool(np.array_equal(res.solved, ref.solved) and np.array_equal(res.lengths, ref.lengths) and
                                 np.array_equal(res.nodes, ref.nodes))
                if rep:
                    secs[cfg].append(dt / calls[cfg])
            print(f"cap {cap} rep {rep} done", flush=True)
        rec = {"serial": {"seconds": spread(secs["serial"])}, "solved": int(ref.solved.sum()), "states": int(ref.nodes.sum()), "pooled": []}
        s_med = rec["serial"]["seconds"]["median"]
        lines.append(f"max_states {cap:7d}: solved {rec['solved']} of {len(states)}, {rec['states']} states;  serial "
                     f"{1e3 * s_med:8.1f} ms [{1e3 * rec['serial']['seconds']['min']:.1f}-{1e3 * rec['serial']['seconds']['max']:.1f}]")
        for cfg in configs:
            S, C, _, _, total = bfs_batch_plan(len(states), cap, cfg[0], cfg[1])
            sp = spread(secs[cfg])
            rec["pooled"].append({"slots": S, "chunk": C, "steps_per_round": cfg[2], "bytes": total, "seconds": sp, "searches_per_timing": calls[cfg],
                                  "identical_to_serial": same[cfg], "serial_over_pooled": round(s_med / sp["median"], 1)})
            lines.append(f"    S {S:5d} C {C:5d} K {cfg[2]}  {total / 2 ** 30:6.2f} GiB  pooled {1e3 * sp['median']:8.2f} ms [{1e3 * sp['min']:.2f}-{1e3 * sp['max']:.2f}]  "
                         f"serial / pooled x{s_med / sp['median']:.1f}  identical {same[cfg]}")
        out["caps"][str(cap)] = rec
        del serial, agents
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
