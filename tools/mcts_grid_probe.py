"""
The reference's MCTS grid search (librubiks/solving/hyper_optim.py: c in (0.1, 100), search_graph=True, iterations 125 -> 125 points,
100 games a point, score = solve share) on one MI355X, trained weights fc_small_r1, deterministic engine, one max_states bound,
one scrambling depth:

  loop      the reference's route: a fresh MCTS and one Evaluator.eval per grid point.  This leg uses nothing but API that predates
            the per-game argument (MCTS, Evaluator(slots=...).eval), so the same leg run on an older checkout is the baseline.
            It also says where its time goes: building the point's forest, building its inference engine (`set_net`),
            `torch.cuda.empty_cache()`, and capturing HIP graphs (every point keys its graphs by its own c: `MCTSForest._graph_key`).
  pooled    GridSearch(pooled=True): the whole grid as one pool (Evaluator.eval_sweep -> MCTS.search_batch with c per game) on
            --slots slots; one captured graph per launch size serves every c.

One leg per call (`--leg loop --name loop_1`), so that a caller can alternate the routes, each under a time limit of its own; every
call merges its record into --out and appends its log to the .txt beside it.  Every leg starts from np.random.seed(0), so all legs
search the same scrambles; the score histories must be identical (the record keeps the list once and a flag per leg).
--iterations below 125 is an evenly spaced subset of the reference's grid (np.linspace over the same interval).

    python tools/mcts_grid_probe.py --out profiles/mcts_grid_probe.json --leg loop --name loop_1
    python tools/mcts_grid_probe.py --out profiles/mcts_grid_probe.json --leg pooled --name pooled_1
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd")]

PARAMETERS = {"c": (0.1, 100)}
LOG = []


def say(*a):
    line = " ".join(str(x) for x in a)
    LOG.append(line)
    print(line, flush=True)


class Stopwatch:
    """Wall seconds spent inside `owner.name`, synchronised on both sides so that the time is the call's own."""

    def __init__(self, owner, name):
        self.owner, self.name, self.inner, self.seconds, self.calls = owner, name, getattr(owner, name), 0.0, 0
        watch = self

        def timed(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            try:
                return watch.inner(*a, **k)
            finally:
                torch.cuda.synchronize()
                watch.seconds += time.perf_counter() - t
                watch.calls += 1
        setattr(owner, name, timed)

    def take(self) -> float:
        s, self.seconds = self.seconds, 0.0
        return round(s, 4)

    def undo(self):
        setattr(self.owner, self.name, self.inner)


class CaptureWatch:
    """Wall seconds inside `with torch.cuda.graph(...)` blocks -- what `MCTSForest.step` / `_graph_of_steps` spend recording an
    iteration they have not got a graph for -- and their number.  The forest has drained the queue before it enters the block, and
    the eager iteration a capturing `step` runs first is part of the search: neither is counted."""

    def __init__(self):
        self.seconds, self.calls = 0.0, 0
        self.inner = (torch.cuda.graph.__enter__, torch.cuda.graph.__exit__)
        watch = self

        def enter(ctx):
            torch.cuda.synchronize()
            watch.t = time.perf_counter()
            return watch.inner[0](ctx)

        def leave(ctx, *exc):
            out = watch.inner[1](ctx, *exc)
            torch.cuda.synchronize()
            watch.seconds += time.perf_counter() - watch.t
            watch.calls += 1
            return out
        torch.cuda.graph.__enter__, torch.cuda.graph.__exit__ = enter, leave

    def take(self) -> float:
        s, self.seconds = self.seconds, 0.0
        return round(s, 4)

    def undo(self):
        torch.cuda.graph.__enter__, torch.cuda.graph.__exit__ = self.inner


def loop_leg(model, iterations, games, depth, cap, slots):
    """Point by point, spelt out with the API of the commit before the per-game argument."""
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    from librubiks.solving.evaluation import Evaluator
    watches = {"forest_alloc": Stopwatch(md.MCTSForest, "__init__"), "set_net": Stopwatch(md.MCTSForest, "set_net"),
               "empty_cache": Stopwatch(torch.cuda, "empty_cache"), "graph_capture": CaptureWatch()}
    parts = {k: [] for k in watches}
    space = np.linspace(*PARAMETERS["c"], iterations)
    ev = Evaluator(games, [depth], None, cap, slots=slots)
    np.random.seed(0)
    scores, per_point = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, c in enumerate(space):
        t = time.perf_counter()
        agent = MCTS(model, c=float(c), search_graph=True, deterministic=True)
        res, states, _ = ev.eval(agent)
        res = res.ravel()
        won = res != -1
        scores.append(float(won.mean()) if won.any() else 0.0)
        torch.cuda.synchronize()
        per_point.append(round(time.perf_counter() - t, 4))
        for k, w in watches.items():
            parts[k].append(w.take())
        del agent
        if (i + 1) % 5 == 0 or i + 1 == len(space):
            say(f"  loop: c {c:.3f} done, {time.perf_counter() - t0:.1f} s so far; the last points took {per_point[-5:]}")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    graphs = watches["graph_capture"].calls
    for w in watches.values():
        w.undo()
    capture = sum(parts["graph_capture"])
    say(f"  loop: of {dt:.1f} s, graph capture {capture:.1f} ({graphs} graphs), forest_alloc {sum(parts['forest_alloc']):.1f}, "
        f"set_net {sum(parts['set_net']):.1f}, empty_cache {sum(parts['empty_cache']):.1f}; median point {float(np.median(per_point)):.2f} s, "
        f"slowest {max(per_point):.2f} s")
    return dt, scores, {"seconds_per_point": per_point, "seconds_per_point_in": parts, "graph_capture_seconds": round(capture, 3),
                        "graphs_captured": graphs}


def pooled_leg(model, iterations, games, depth, cap, slots):
    from librubiks.solving.agents import MCTS
    from librubiks.solving.evaluation import Evaluator
    from librubiks.solving.hyper_optim import GridSearch
    watch = CaptureWatch()
    ev = Evaluator(games, [depth], None, cap, slots=slots)
    gs = GridSearch(None, PARAMETERS, pooled=True)
    gs.objective_from_evaluator(ev, MCTS, {"net": model, "search_graph": True, "deterministic": True})
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gs.optimize(iterations)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    capture, graphs = watch.take(), watch.calls
    watch.undo()
    say(f"  pooled: of {dt:.1f} s, the search {ev.batch_seconds[0]:.1f}, graph capture {capture:.1f} ({graphs} graphs)")
    return dt, [float(s) for s in gs.score_history], {"search_seconds": round(ev.batch_seconds[0], 3), "graph_capture_seconds": round(capture, 3),
                                                      "graphs_captured": graphs, "optimal": {k: float(v) for k, v in gs.optimal.items()},
                                                      "highscore": float(gs.highscore)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="mcts_grid_probe.json")
    ap.add_argument("--leg", choices=("loop", "pooled"), required=True)
    ap.add_argument("--name", default=None, help="the record's key for this leg (default: the leg's name)")
    ap.add_argument("--iterations", type=int, default=125)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--max-states", type=int, default=50_000)
    ap.add_argument("--slots", type=int, default=4096)
    args = ap.parse_args()
    name = args.name or args.leg
    from librubiks.model import Model
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    settings = {k: v for k, v in vars(args).items() if k not in ("out", "leg", "name")}
    out = {"args": settings, "device": torch.cuda.get_device_name(0), "weights": "fc_small_r1", "deterministic": True, "search_graph": True}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        if old.get("args") == settings:     # the legs of one measurement share a record; other settings start a new one
            out = old
    say(f"{name}: {args.iterations} of the reference's 125 points, c {np.linspace(*PARAMETERS['c'], args.iterations).round(3).tolist()}; "
        f"{args.games} games a point at depth {args.depth}, max_states {args.max_states}, {args.slots} slots, {out['device']}")
    dt, scores, extra = (loop_leg if args.leg == "loop" else pooled_leg)(model, args.iterations, args.games, args.depth, args.max_states, args.slots)
    first = out.setdefault("scores", scores)
    out[name] = {"route": args.leg, "seconds": round(dt, 3), "scores_identical_to_the_recorded_list": scores == first, **extra}
    say(f"{name}: {dt:.2f} s, best score {max(scores):.3f} at point {int(np.argmax(scores))}, {sum(s > 0 for s in scores)} of {len(scores)} points solve something")
    legs = [k for k, v in out.items() if isinstance(v, dict) and "route" in v]
    if len(legs) > 1:
        out["histories_identical"] = all(out[k]["scores_identical_to_the_recorded_list"] for k in legs)
        say("score histories identical between", legs, ":", out["histories_identical"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        text = json.dumps(out, indent=1)
        f.write(re.sub(r"\[[^\[\]{}]*\]", lambda m: " ".join(m.group(0).split()), text) + "\n")   # a list of numbers on one line
    with open(os.path.splitext(args.out)[0] + ".txt", "a") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
