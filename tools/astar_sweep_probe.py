"""
The reference's A* grid search (librubiks/solving/hyper_optim.py: lambda_ in (0, 0.4) x expansions in (1, 1000), iterations 125 ->
11 x 11 points, 100 games a point, score = solve share / mean length) on one MI355X, trained weights fc_small_r1, deterministic
engine, one max_states bound, one scrambling depth:

  loop      the reference's route: a fresh AStar and one Evaluator.eval per grid point.  This leg uses nothing but API that predates
            the per-game arguments (AStar, Evaluator(slots=...).eval), so the same leg run on an older checkout is the baseline.
  pooled    GridSearch(pooled=True): the whole grid as one pool (Evaluator.eval_sweep -> AStar.search_batch with per-game lambda_
            and expansions) on --slots slots, planted by descending expansions (AStar.plant_order's default)
  given     the same with AStar.plant_order = "given" (the caller's point-major order)
  loop_again, pooled_again   the two routes once more, so that each is timed twice, alternated (loop, pooled, loop, pooled)
  order     `pooled` against `given` on a reduced grid (--order-iterations, --order-games, --order-slots), for when the full grid
            in the caller's order does not fit a visit

Every leg starts from np.random.seed(0), so all legs search the same scrambles; the score histories must be identical (the record
keeps the list once and a flag per leg).  The loop legs also say where a point's time goes: building the point's AStarBatch (its
arrays are allocated and zeroed up front), building its inference engine (`set_net`), `torch.cuda.empty_cache()`, and the rest
(scrambles, the search itself, result extraction).

    python tools/astar_sweep_probe.py --out profiles/astar_sweep_probe.json      (writes the .txt log beside it)
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

PARAMETERS = {"lambda_": (0, 0.4), "expansions": (1, 1000)}
LOG = []


def say(*a):
    line = " ".join(str(x) for x in a)
    LOG.append(line)
    print(line, flush=True)


def prep(params):
    params["expansions"] = int(params["expansions"])
    return params


class Stopwatch:
    """Wall seconds spent inside `owner.name`, synchronised on both sides so that the time is the call's own."""

    def __init__(self, owner, name):
        self.owner, self.name, self.inner, self.seconds = owner, name, getattr(owner, name), 0.0
        watch = self

        def timed(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            try:
                return watch.inner(*a, **k)
            finally:
                torch.cuda.synchronize()
                watch.seconds += time.perf_counter() - t
        setattr(owner, name, timed)

    def take(self) -> float:
        s, self.seconds = self.seconds, 0.0
        return round(s, 4)

    def undo(self):
        setattr(self.owner, self.name, self.inner)


def loop_leg(model, iterations, games, depth, cap, slots):
    """Point by point, spelt out with the API of the commit before the per-game arguments."""
    from librubiks.solving import astar_device as ad
    from librubiks.solving.agents import AStar
    from librubiks.solving.evaluation import Evaluator
    watches = {"batch_alloc": Stopwatch(ad.AStarBatch, "__init__"), "set_net": Stopwatch(ad.AStarBatch, "set_net"),
               "empty_cache": Stopwatch(torch.cuda, "empty_cache")}
    parts = {k: [] for k in watches}
    n = int(iterations ** (1 / len(PARAMETERS)) + 1e-6)
    spaces = [np.linspace(*interval, n) for interval in PARAMETERS.values()]
    ev = Evaluator(games, [depth], None, cap, slots=slots)
    np.random.seed(0)
    scores, per_point = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        for j in range(n):
            t = time.perf_counter()
            agent = AStar(model, lambda_=float(spaces[0][i]), expansions=int(spaces[1][j]), deterministic=True)
            res, states, _ = ev.eval(agent)
            res = res.ravel()
            won = res != -1
            share = won.mean() if won.any() else 0
            scores.append(float(share / res[won].mean()) if share else 0.0)
            torch.cuda.synchronize()
            per_point.append(round(time.perf_counter() - t, 4))
            for k, w in watches.items():
                parts[k].append(w.take())
            del agent
        say(f"  loop: lambda {spaces[0][i]:.2f} done, {time.perf_counter() - t0:.1f} s so far; this row's points took {per_point[-n:]}")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for w in watches.values():
        w.undo()
    slow = [i for i, x in enumerate(per_point) if x > 3 * float(np.median(per_point))]
    say(f"  loop: of {dt:.1f} s, batch_alloc {sum(parts['batch_alloc']):.1f}, set_net {sum(parts['set_net']):.1f}, empty_cache {sum(parts['empty_cache']):.1f}; "
        f"{len(slow)} points above 3 x the median point ({float(np.median(per_point)):.2f} s) take {sum(per_point[i] for i in slow):.1f} s: in them "
        f"batch_alloc {sum(parts['batch_alloc'][i] for i in slow):.1f}, set_net {sum(parts['set_net'][i] for i in slow):.1f}, "
        f"empty_cache {sum(parts['empty_cache'][i] for i in slow):.1f} s")
    return dt, scores, {"seconds_per_point": per_point, "seconds_per_point_in": parts, "slow_points": slow}


def pooled_leg(model, iterations, games, depth, cap, slots, order):
    from librubiks.solving.agents import AStar
    from librubiks.solving.evaluation import Evaluator
    from librubiks.solving.hyper_optim import GridSearch
    ev = Evaluator(games, [depth], None, cap, slots=slots)
    gs = GridSearch(None, PARAMETERS, pooled=True)

    class Ordered(AStar):
        plant_order = order
    gs.objective_from_evaluator(ev, Ordered, {"net": model, "deterministic": True}, param_prepper=prep, optim_lengths=True)
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gs.optimize(iterations)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, [float(s) for s in gs.score_history], {"search_seconds": round(ev.batch_seconds[0], 3), "optimal": {k: float(v) for k, v in gs.optimal.items()},
                                                      "highscore": float(gs.highscore)}


def run(name, fn, out, *a):
    say(f"{name}: start")
    dt, scores, extra = fn(*a)
    first = out.setdefault("scores" if len(scores) == len(out.get("scores", scores)) else "scores_reduced_grid", scores)
    out[name] = {"seconds": round(dt, 3), "scores_identical_to_the_recorded_list": scores == first, **extra}
    say(f"{name}: {dt:.2f} s, best score {max(scores):.5f} at point {int(np.argmax(scores))}, {sum(s > 0 for s in scores)} of {len(scores)} points solve something")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="astar_sweep_probe.json")
    ap.add_argument("--legs", default="loop,pooled,loop_again,pooled_again,given,order")
    ap.add_argument("--iterations", type=int, default=125)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--max-states", type=int, default=50_000)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--order-iterations", type=int, default=25)
    ap.add_argument("--order-games", type=int, default=40)
    ap.add_argument("--order-slots", type=int, default=256)
    args = ap.parse_args()
    from librubiks.model import Model
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    out = {"args": {k: v for k, v in vars(args).items() if k != "out"}, "device": torch.cuda.get_device_name(0), "weights": "fc_small_r1",
           "deterministic": True}
    n = int(args.iterations ** 0.5 + 1e-6)
    say(f"grid {n} x {n}: lambda_ {np.linspace(0, 0.4, n).round(3).tolist()}, expansions {[int(x) for x in np.linspace(1, 1000, n)]}; "
        f"{args.games} games a point at depth {args.depth}, max_states {args.max_states}, {args.slots} slots, {out['device']}")
    full = (model, args.iterations, args.games, args.depth, args.max_states, args.slots)
    small = (model, args.order_iterations, args.order_games, args.depth, args.max_states, args.order_slots)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            text = json.dumps(out, indent=1)
            f.write(re.sub(r"\[[^\[\]{}]*\]", lambda m: " ".join(m.group(0).split()), text) + "\n")   # a list of numbers on one line
        with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
            f.write("\n".join(LOG) + "\n")
    for leg in args.legs.split(","):
        if leg in ("loop", "loop_again"):
            run(leg, loop_leg, out, *full)
        elif leg in ("pooled", "pooled_again", "given"):
            run(leg, pooled_leg, out, *full, "given" if leg == "given" else "descending")
        elif leg == "order":
            m = int(args.order_iterations ** 0.5 + 1e-6)
            say(f"order: reduced grid {m} x {m}, {args.order_games} games a point, {args.order_slots} slots")
            for name, order in (("order_descending", "descending"), ("order_given", "given"), ("order_descending_again", "descending")):
                run(name, pooled_leg, out, *small, order)
            out["order_histories_identical"] = all(out[k]["scores_identical_to_the_recorded_list"] for k in ("order_descending", "order_given", "order_descending_again"))
            say("order: score histories identical:", out["order_histories_identical"])
        torch.cuda.empty_cache()
        have = [k for k in ("loop", "pooled", "loop_again", "pooled_again", "given") if k in out]
        if len(have) > 1:
            out["histories_identical"] = all(out[k]["scores_identical_to_the_recorded_list"] for k in have)
            say("score histories identical between", have, ":", out["histories_identical"])
        save()
    save()


if __name__ == "__main__":
    main()
