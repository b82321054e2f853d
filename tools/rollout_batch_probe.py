"""
The one-step agents (greedy policy, sampled policy, greedy value, random) in lock step on the device against the batched search
that is driven move by move from the host, on one MI355X, trained weights fc_small_r1.  The games are those of the evaluation
protocol of tools/astar_pool_probe.py (500 games x depths 10,15,20,25,30) at max_states 200, on the f32s and bf16 engines.

  stepwise    `search_batch(states, None, cap)` per depth: the path without keywords (unchanged by the lock-step search)
  lockstep    `search_batch(states, None, cap, seeds=...)` per depth
  pool_S      all depths as one pool on S slots: `search_batch(pool, None, cap, seeds=..., slots=S)`

The forms alternate within one process after a warm-up run of every form; the median of the repetitions is reported with their
minimum and maximum.  For the lock-step forms the host's draw time per round stands beside the device time of a round.
`--steps-per-round` takes a list: the lock-step form per depth is then measured at every value.

    python tools/rollout_batch_probe.py --out profiles/rollout_batch_probe.json > profiles/rollout_batch_probe.txt
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

DEPTHS = [10, 15, 20, 25, 30]
KINDS = ("greedy", "sampled", "value", "random")


def spread(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "runs": [round(x, 4) for x in xs]}


def make_agent(kind, net, dtype, steps_per_round=None):
    from librubiks.solving.agents import PolicySearch, RandomSearch, ValueSearch
    if kind == "random":
        agent = RandomSearch()
    elif kind == "value":
        agent = ValueSearch(net, net_dtype=dtype)
    else:
        agent = PolicySearch(net, sample_policy=kind == "sampled", net_dtype=dtype)
    if steps_per_round:
        agent.steps_per_round = int(steps_per_round)
    return agent


def scrambles(games, depths, seed=0):
    """One device batch of `games` scrambles per depth, drawn in the Evaluator's order."""
    from librubiks import cube
    np.random.seed(seed)
    return [cube.scramble_batch(games, d, True)[0] for d in depths]


def pooled(batches):
    from librubiks.cube.device import DeviceCubes
    pool = DeviceCubes.empty(sum(b.n for b in batches))
    at = 0
    for b in batches:
        pool.soa[:, at:at + b.n] = b.soa[:, :b.n]
        at += b.n
    return pool


def run(agent, form, batches, cap):
    """-> (seconds, moves made, games solved, host draw seconds, device seconds in rounds) of one run of `form`."""
    draw = device = 0.0
    moves = solved = 0
    np.random.seed(1)                 # the stepwise form draws from the global stream
    todo = batches if form in ("stepwise", "lockstep") else [pooled(batches)]
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i, cubes in enumerate(todo):
        if form == "stepwise":
            res = agent.search_batch(cubes, None, cap)
        else:
            res = agent.search_batch(cubes, None, cap, seeds=i, slots=None if form == "lockstep" else int(form.split("_")[1]))
            draw += agent.batch_stats["draw_s"]
            device += sum(agent.batch_stats["device_round_ms"]) / 1e3
        moves += int(res.nodes.sum())
        solved += int(res.solved.sum())
    torch.cuda.synchronize()
    return time.perf_counter() - t, moves, solved, draw, device


def compare(agent, forms, batches, cap, reps=3, log=None):
    """{form: {"seconds": spread, ...}}: `reps` alternating runs of every form after one warm-up run of each."""
    rows = {f: [] for f in forms}
    for rep in range(reps + 1):
        for f in forms:
            row = run(agent, f, batches, cap)
            if rep:
                rows[f].append(row)
            if log:
                log(f"{f} rep {rep}: {row[0]:.4f} s, {row[1]} moves, {row[2]} solved, draw {row[3] * 1e3:.1f} ms, device rounds {row[4] * 1e3:.1f} ms")
    out = {}
    for f, v in rows.items():
        out[f] = {"seconds": spread([r[0] for r in v]), "M_moves_per_s": spread([r[1] / r[0] / 1e6 for r in v]),
                  "moves": v[0][1], "solved": v[0][2]}
        if f != "stepwise":
            out[f]["host_draw_s"], out[f]["device_round_s"] = spread([r[3] for r in v]), spread([r[4] for r in v])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="rollout_batch_probe.json")
    ap.add_argument("--games", type=int, default=500)
    ap.add_argument("--max-states", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--engines", default="f32s,bf16")
    ap.add_argument("--pools", default="1024,2048")
    ap.add_argument("--steps-per-round", default="4,8,16")
    args = ap.parse_args()
    from librubiks.model import F32_SPLIT, Model
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    engines = {"f32s": F32_SPLIT, "bf16": torch.bfloat16}
    batches = scrambles(args.games, DEPTHS)
    out = {"args": {k: v for k, v in vars(args).items() if k != "out"}, "device": torch.cuda.get_device_name(0), "results": {}}
    forms = ["stepwise", "lockstep"] + [f"pool_{s}" for s in args.pools.split(",") if s]
    for kind in args.kinds.split(","):
        for eng in (["none"] if kind == "random" else args.engines.split(",")):
            res = out["results"].setdefault(kind, {}).setdefault(eng, {})
            say = lambda msg: print(kind, eng, msg, flush=True)   # noqa: E731
            res["forms"] = compare(make_agent(kind, model, engines.get(eng)), forms, batches, args.max_states, args.reps, say)
            res["lockstep_by_steps_per_round"] = {}
            for K in args.steps_per_round.split(","):
                got = compare(make_agent(kind, model, engines.get(eng), K), ["lockstep"], batches, args.max_states, args.reps,
                              lambda msg: say(f"K {K} " + msg))
                res["lockstep_by_steps_per_round"][K] = got["lockstep"]
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
