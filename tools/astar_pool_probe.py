"""
A* continuous batching (`AStar.search_batch(..., slots=S)`) against plain batches, on one MI355X, trained weights fc_small_r1,
lambda 0.2, N 100.  Each A/B alternates its forms within one process, after a warm-up run of every form; the spread is shown.

  eval       the reference's evaluation protocol (500 games x depths 10,15,20,25,30, max_states 175 000): one batch per depth
             (Evaluator without slots) against one pool of all 2 500 games on 1 024 / 2 048 / 2 500 slots, f32s and bf16; then
             the deterministic engine's per-game outcomes of both forms, which must be identical
  configs2   8 x 4 096 depth-20 scrambles on 4 096 slots against eight plain 4 096-problem batches back to back (f32s)
  readback   solution extraction of a solved 4 096-problem batch: the per-problem host walk (two blocking copies per problem)
             against rc_astar_solutions

    python tools/astar_pool_probe.py --out astar_pool_probe.json
"""
import argparse
import json
import os
import sys
import time
from collections import deque

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd")]

DEPTHS = [10, 15, 20, 25, 30]


def spread(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "runs": [round(x, 4) for x in xs]}


def eval_once(agent, slots, games, cap):
    from librubiks.solving.evaluation import Evaluator
    np.random.seed(0)
    ev = Evaluator(games, DEPTHS, None, cap, slots=slots)
    torch.cuda.synchronize()
    t = time.perf_counter()
    res, states, _ = ev.eval(agent)
    torch.cuda.synchronize()
    return time.perf_counter() - t, res, states


def eval_leg(model, args, out):
    from librubiks.model import F32_SPLIT
    from librubiks.solving.agents import AStar
    forms = [None, 1024, 2048, 2500]
    name = lambda s: "per_depth" if s is None else f"pool_{s}"   # noqa: E731
    for dt_name, dt in (("f32s", F32_SPLIT), ("bf16", torch.bfloat16)):
        agent = AStar(model, lambda_=0.2, expansions=100, net_dtype=dt)
        secs = {name(s): [] for s in forms}
        rate = {name(s): [] for s in forms}
        for rep in range(args.reps + 1):                  # rep 0: warm-up of every form
            for s in forms:
                dt_s, res, states = eval_once(agent, s, args.games, args.max_states)
                if rep:
                    secs[name(s)].append(dt_s)
                    rate[name(s)].append(states.sum() / dt_s / 1e6)
                print(dt_name, name(s), f"rep {rep}: {dt_s:.3f} s, {states.sum() / dt_s / 1e6:.2f} M states/s, solved {(res >= 0).mean():.4f}", flush=True)
        out["eval"][dt_name] = {k: {"seconds": spread(secs[k]), "M_states_per_s": spread(rate[k])} for k in secs}
        del agent
        torch.cuda.empty_cache()
    det = AStar(model, lambda_=0.2, expansions=100, deterministic=True)
    _, r0, s0 = eval_once(det, None, args.games, args.max_states)
    _, r1, s1 = eval_once(det, 1024, args.games, args.max_states)
    out["eval"]["deterministic_outcomes_identical"] = bool(np.array_equal(r0, r1) and np.array_equal(s0, s1))
    print("deterministic per-depth vs pool_1024 identical:", out["eval"]["deterministic_outcomes_identical"], flush=True)
    del det
    torch.cuda.empty_cache()


def configs2_leg(model, args, out):
    from librubiks import cube
    from librubiks.model import F32_SPLIT
    from librubiks.solving.agents import AStar
    B, K = 4096, args.batches
    np.random.seed(1)
    cubes, _, _ = cube.scramble_batch(B * K, 20, True)
    states = cubes.numpy()
    agent = AStar(model, lambda_=0.2, expansions=100, net_dtype=F32_SPLIT)
    agent.search_batch(states[:B], None, args.max_states, max_iterations=3)      # warm-up: engine, batch, plans
    rows = {"plain": [], "pool": []}
    for rep in range(args.reps):
        for form in ("plain", "pool"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if form == "plain":
                nodes = sum(int(agent.search_batch(states[i * B:(i + 1) * B], None, args.max_states).nodes.sum()) for i in range(K))
            else:
                nodes = int(agent.search_batch(states, None, args.max_states, slots=B).nodes.sum())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            rows[form].append((dt, nodes / dt / 1e6))
            print(f"configs2 {form} rep {rep}: {dt:.3f} s, {nodes} states, {nodes / dt / 1e6:.2f} M states/s", flush=True)
    out["configs2"] = {f: {"seconds": spread([r[0] for r in v]), "M_states_per_s": spread([r[1] for r in v])} for f, v in rows.items()}
    out["configs2"]["scrambles"], out["configs2"]["slots"] = B * K, B
    del agent
    torch.cuda.empty_cache()


def host_loop(batch):
    """The parent commit's per-problem extraction: two blocking copies and a Python walk per solved problem."""
    from librubiks.solving import astar_device as ad
    status = batch.status.cpu().numpy()
    nodes = batch.n_nodes.cpu().numpy().astype(np.int64)
    sol_idx = batch.solved_idx.cpu().numpy()
    queues = []
    for b in range(batch.B):
        q = deque()
        if status[b] == ad.SOLVED:
            lo = b * (batch.C + 1)
            par = batch.parents[lo:lo + nodes[b] + 1].cpu().numpy()
            pact = batch.parent_actions[lo:lo + nodes[b] + 1].cpu().numpy()
            i = int(sol_idx[b])
            while i != 1:
                q.appendleft(int(pact[i]))
                i = int(par[i])
        queues.append(q)
    return queues


def readback_leg(model, args, out):
    from librubiks import cube
    from librubiks.model import F32_SPLIT
    from librubiks.solving.agents import AStar
    np.random.seed(2)
    cubes, _, _ = cube.scramble_batch(4096, 20, True)
    agent = AStar(model, lambda_=0.2, expansions=100, net_dtype=F32_SPLIT)
    res = agent.search_batch(cubes, None, args.max_states)
    batch = agent.batch
    every = np.arange(batch.B)
    rows = {"host_loop": [], "rc_astar_solutions": []}
    for rep in range(args.reps + 1):
        for form in rows:
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = host_loop(batch) if form == "host_loop" else batch.solutions(every)[1]
            dt = time.perf_counter() - t
            if rep:
                rows[form].append(dt)
            same = all(list(got[b]) == list(res.queues[b]) for b in range(batch.B))
            print(f"readback {form} rep {rep}: {dt * 1e3:.2f} ms, equal to the search's queues: {same}", flush=True)
            assert same
    out["readback"] = {k: {"ms": spread([x * 1e3 for x in v])} for k, v in rows.items()}
    out["readback"]["solved"] = int(res.solved.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="astar_pool_probe.json")
    ap.add_argument("--legs", default="eval,configs2,readback")
    ap.add_argument("--games", type=int, default=500)
    ap.add_argument("--max-states", type=int, default=175_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batches", type=int, default=8)
    args = ap.parse_args()
    from librubiks.model import Model
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    out = {"eval": {}, "args": {k: v for k, v in vars(args).items() if k != "out"}, "device": torch.cuda.get_device_name(0)}
    legs = {"eval": eval_leg, "configs2": configs2_leg, "readback": readback_leg}
    for leg in args.legs.split(","):
        legs[leg](model, args, out)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
