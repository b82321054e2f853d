"""
What `shorten=True` does to the solutions of the agents that walk -- EGVM, the sampled policy, RandomSearch -- and what it costs,
on one MI355X, trained weights fc_small_r1 (librubiks/solving/shorten.py, csrc/rubiks_shorten.hip).

  egvm      api.py's parameters (eps 0.375, W 10, D 50) on 1 024 depth-20 scrambles at max_states 50 000, lock step
            (`search_batch(..., seeds=)`), on the f32s and bf16 engines
  sampled   PolicySearch(sample_policy=True) and
  random    RandomSearch on the games of the evaluation protocol of tools/rollout_batch_probe.py (500 games x depths 10, 15, 20, 25,
            30 as one pool) at max_states 200, lock step

Per case: the solved share; mean / median / max length of the solved games' queues as searched and as shortened and the share
of solved games that got shorter; the wall seconds of the search (median [min-max] of --reps runs after a warm-up run) and of
`BatchResult.shortened` on its result (upload, the three launches, read-back; --shorten-reps runs after a warm-up), the device
time of each of the three launches (HIP events around each, summed over the chunks), the workspace bytes and the number of chunks.

    python tools/shorten_probe.py --out profiles/shorten_probe.json      (writes the .txt beside it)
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

EPS, W, D = 0.375, 10, 50
DEPTHS = [10, 15, 20, 25, 30]


def spread(xs, digits=4):
    xs = sorted(float(x) for x in xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def fmt(s, unit=""):
    return f"{s['median']}{unit} [{s['min']}-{s['max']}]"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, res


def lengths_of(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean": round(float(x.mean()), 2), "median": float(np.median(x)), "max": int(x.max())} if len(x) else None


def measure(name, search, states, args, out, lines):
    """search() -> BatchResult (shorten=False); the shortening is timed apart on its result."""
    from librubiks.solving import shorten as sh
    secs = []
    for rep in range(args.reps + 1):                          # rep 0: warm-up
        dt, res = timed(search)
        if rep:
            secs.append(dt)
    won = np.asarray(res.solved, dtype=bool) & (res.lengths > 0)
    if not won.any():
        out["cases"][name] = {"games": int(len(res.solved)), "solved_share": round(float(np.mean(res.solved)), 4), "solved_with_moves": 0,
                              "search_seconds": spread(secs)}
        lines.append(f"{name:14s} games {len(res.solved):5d} solved {np.mean(res.solved):.4f}: no solved game with moves, nothing to shorten; "
                     f"search {fmt(spread(secs), ' s')}")
        print(lines[-1], flush=True)
        return
    wall, launches, info = [], {k: [] for k in sh.STEPS}, {}
    for rep in range(args.shorten_reps + 1):
        dt, short = timed(lambda: res.shortened(states))
        timings = {}
        sh.shorten_queues(states, res.queues, select=won, timings=timings, info=info)
        torch.cuda.synchronize()
        if rep:
            wall.append(dt)
            for k in sh.STEPS:
                launches[k].append(sum(a.elapsed_time(b) for a, b in timings[k]))
    raw, cut = res.lengths[won], short.lengths[won]
    rec = {"games": int(len(res.solved)), "solved_share": round(float(np.mean(res.solved)), 4), "solved_with_moves": int(won.sum()),
           "raw_length": lengths_of(raw), "short_length": lengths_of(cut),
           "share_shorter": round(float(np.mean(cut < raw)), 4) if won.any() else None,
           "positions": int((raw + 1).sum()),
           "search_seconds": spread(secs), "shorten_seconds": spread(wall),
           "launch_ms": {k: spread(v, 3) for k, v in launches.items()},
           "workspace_bytes": int(info.get("workspace_bytes", 0)), "chunks": int(info.get("chunks", 0))}
    rec["shorten_over_search"] = round(rec["shorten_seconds"]["median"] / rec["search_seconds"]["median"], 4)
    out["cases"][name] = rec
    lines.append(f"{name:14s} games {rec['games']:5d} solved {rec['solved_share']:.4f}  raw mean/median/max "
                 f"{rec['raw_length']['mean']}/{rec['raw_length']['median']}/{rec['raw_length']['max']}  short "
                 f"{rec['short_length']['mean']}/{rec['short_length']['median']}/{rec['short_length']['max']}  got shorter {rec['share_shorter']}")
    lines.append(f"{'':14s} search {fmt(rec['search_seconds'], ' s')}  shortened() {fmt(rec['shorten_seconds'], ' s')} "
                 f"= {rec['shorten_over_search']} of the search;  launches: " +
                 ", ".join(f"{k[len('rc_shorten_'):]} {fmt(v, ' ms')}" for k, v in rec["launch_ms"].items()) +
                 f";  {rec['positions']} positions, workspace {rec['workspace_bytes'] / 2 ** 20:.1f} MiB, {rec['chunks']} chunk(s)")
    print("\n".join(lines[-2:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/shorten_probe.json")
    ap.add_argument("--cases", default="egvm_f32s,egvm_bf16,sampled,random")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--eval-games", type=int, default=500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shorten-reps", type=int, default=5)
    args = ap.parse_args()
    from librubiks import cube
    from librubiks.model import F32_SPLIT, Model
    from librubiks.solving.agents import EGVM, PolicySearch, RandomSearch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from rollout_batch_probe import pooled, scrambles
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    out = {"cases": {}, "args": {k: v for k, v in vars(args).items() if k != "out"}, "device": torch.cuda.get_device_name(0)}
    lines = [f"shorten=True: lengths and cost, fc_small_r1; search: {args.reps} runs after a warm-up, shortening: {args.shorten_reps} runs "
             f"after a warm-up (median [min-max]); {out['device']}"]
    for name in args.cases.split(","):
        if name.startswith("egvm"):
            np.random.seed(1)
            states = cube.scramble_batch(args.games, 20, True)[0]
            seeds = np.random.randint(0, 2 ** 31 - 1, args.games)
            agent = EGVM(model, EPS, W, D, net_dtype=F32_SPLIT if name.endswith("f32s") else torch.bfloat16)
            search = lambda: agent.search_batch(states, None, 50_000, seeds=seeds)   # noqa: E731
        else:
            states = pooled(scrambles(args.eval_games, DEPTHS))
            agent = RandomSearch() if name == "random" else PolicySearch(model, sample_policy=True, net_dtype=F32_SPLIT)
            search = lambda: agent.search_batch(states, None, 200, seeds=1)          # noqa: E731
        measure(name, search, states, args, out, lines)
        del agent
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
