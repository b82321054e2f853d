"""
EGVM: the batched search (`EGVM.search_batch(..., seeds=)`, all games in lock step on the device) against the serial form (one
`search` after the other), on one MI355X, trained weights fc_small_r1, depth-20 scrambles, eps 0.375.  The forms alternate within
one process after a warm-up run of each; medians and min-max are shown.

  sizes    api.py's parameters (W 10, D 50, max_states 50 000) with 64 and 1 024 games, and the evaluation config's W 500, D 250
           (max_states 500 000: four rounds) with 64 games; f32s and bf16.  States explored per second and wall time of both forms,
           and per round of the batched form: the host's drawing time beside the device time of the round.
           The serial form takes about 10 ms per game and round at W 10 (2 D host round trips), so it is timed on the first
           --serial-games games of each set (its rate does not depend on how many games follow one another); the batched form
           runs all of them.
  parity   128 depth-12 scrambles, W 10, D 50, max_states 20 000: solve rates of both forms on the same games and per-game seeds,
           and the share of games that end identically (solved flag, states, action queue).

    python tools/egvm_batch_probe.py --out profiles/egvm_batch_probe.json      (writes the .txt beside it)
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

EPS = 0.375
SIZES = {"api_64": dict(games=64, W=10, D=50, cap=50_000), "api_1024": dict(games=1024, W=10, D=50, cap=50_000),
         "eval_64": dict(games=64, W=500, D=250, cap=500_000)}


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def scrambles(n, depth, seed):
    from librubiks import cube
    np.random.seed(seed)
    cubes, _, _ = cube.scramble_batch(n, depth, True)
    return cubes.numpy(), np.random.randint(0, 2 ** 31 - 1, n)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, res


def sizes_leg(model, args, out, lines):
    from librubiks.model import F32_SPLIT
    from librubiks.solving.agents import EGVM
    for dt_name, dt in (("f32s", F32_SPLIT), ("bf16", torch.bfloat16)):
        for name in args.sizes.split(","):
            cfg = SIZES[name]
            states, seeds = scrambles(cfg["games"], 20, 1)
            n_serial = min(args.serial_games, cfg["games"])
            agent = EGVM(model, EPS, cfg["W"], cfg["D"], net_dtype=dt)
            rows = {"serial": [], "batched": []}
            rounds = []
            for rep in range(args.reps + 1):                  # rep 0: warm-up of both forms
                np.random.seed(rep)
                dt_s, res_s = timed(lambda: agent.search_batch(states[:2 if rep == 0 else n_serial], None, cfg["cap"]))
                dt_b, res_b = timed(lambda: agent.search_batch(states, None, cfg["cap"], seeds=seeds))
                st = agent.batch_stats
                print(f"{dt_name} {name} rep {rep}: serial {dt_s:.3f} s ({res_s.nodes.sum() / dt_s / 1e3:.1f} k states/s), batched "
                      f"{dt_b:.3f} s ({res_b.nodes.sum() / dt_b / 1e3:.1f} k states/s), {st['rounds']} rounds", flush=True)
                if rep:
                    rows["serial"].append((dt_s, res_s.nodes.sum() / dt_s))
                    rows["batched"].append((dt_b, res_b.nodes.sum() / dt_b))
                    rounds.append({"rounds": st["rounds"], "draw_ms_per_round": 1e3 * st["draw_s"] / max(1, st["rounds"]),
                                   "device_ms_per_round": float(np.median(st["device_round_ms"][1:] or st["device_round_ms"])),
                                   "host_wait_s": st["wait_s"], "draw_not_overlapped_s": st["draw_exposed_s"]})
            rec = {"games": cfg["games"], "serial_games": n_serial, "workers": cfg["W"], "depth": cfg["D"], "max_states": cfg["cap"],
                   "solved_batched": int(res_b.solved.sum()),
                   "serial": {"seconds": spread([r[0] for r in rows["serial"]]), "states_per_s": spread([r[1] for r in rows["serial"]])},
                   "batched": {"seconds": spread([r[0] for r in rows["batched"]]), "states_per_s": spread([r[1] for r in rows["batched"]])},
                   "per_round": {k: spread([r[k] for r in rounds]) for k in rounds[0]}}
            rec["rate_ratio"] = round(rec["batched"]["states_per_s"]["median"] / rec["serial"]["states_per_s"]["median"], 1)
            out["sizes"].setdefault(dt_name, {})[name] = rec
            pr = rec["per_round"]
            lines.append(f"{dt_name:5s} {name:9s} games {cfg['games']:5d} W {cfg['W']:3d} D {cfg['D']:3d}  serial ({n_serial} games) "
                         f"{rec['serial']['seconds']['median']:8.3f} s {rec['serial']['states_per_s']['median'] / 1e3:9.1f} k st/s "
                         f"[{rec['serial']['states_per_s']['min'] / 1e3:.1f}-{rec['serial']['states_per_s']['max'] / 1e3:.1f}]   batched "
                         f"{rec['batched']['seconds']['median']:8.3f} s {rec['batched']['states_per_s']['median'] / 1e3:9.1f} k st/s "
                         f"[{rec['batched']['states_per_s']['min'] / 1e3:.1f}-{rec['batched']['states_per_s']['max'] / 1e3:.1f}]  x{rec['rate_ratio']}"
                         f"   per round: draw {pr['draw_ms_per_round']['median']:.2f} ms, device {pr['device_ms_per_round']['median']:.2f} ms")
            del agent
            torch.cuda.empty_cache()


def parity_leg(model, args, out, lines):
    from librubiks.model import F32_SPLIT
    from librubiks.solving.agents import EGVM
    from oracle import cube as oc
    np.random.seed(12)
    states = np.array([oc.scramble(12, True)[0] for _ in range(128)])
    seeds = np.random.randint(0, 2 ** 31 - 1, 128)
    W, D, cap = 10, 50, 20_000
    for dt_name, dt in (("f32s", F32_SPLIT), ("bf16", torch.bfloat16)):
        agent = EGVM(model, EPS, W, D, net_dtype=dt)
        agent.search_batch(states, None, cap, seeds=seeds)   # warm-up
        dt_b, res = timed(lambda: agent.search_batch(states, None, cap, seeds=seeds))
        serial = []
        t0 = time.perf_counter()
        for s, seed in zip(states, seeds):
            np.random.seed(int(seed))
            ok = agent.search(s, None, cap)
            serial.append((bool(ok), len(agent), list(agent.action_queue)))
        dt_s = time.perf_counter() - t0
        got = [(bool(res.solved[g]), int(res.nodes[g]), list(res.queues[g])) for g in range(128)]
        rec = {"solve_rate_serial": float(np.mean([w[0] for w in serial])), "solve_rate_batched": float(res.solved.mean()),
               "games_identical": float(np.mean([a == b for a, b in zip(got, serial)])), "seconds_serial": round(dt_s, 3),
               "seconds_batched": round(dt_b, 3)}
        out["parity"][dt_name] = rec
        lines.append(f"parity {dt_name}: 128 depth-12 games, W 10, D 50, max_states 20 000: solve rate serial {rec['solve_rate_serial']:.4f}, "
                     f"batched {rec['solve_rate_batched']:.4f}; games identical to the serial search {rec['games_identical']:.4f}; "
                     f"wall serial {dt_s:.2f} s, batched {dt_b:.3f} s")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/egvm_batch_probe.json")
    ap.add_argument("--legs", default="sizes,parity")
    ap.add_argument("--sizes", default="api_64,api_1024,eval_64")
    ap.add_argument("--serial-games", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    from librubiks.model import Model
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    out = {"sizes": {}, "parity": {}, "args": {k: v for k, v in vars(args).items() if k != "out"}, "device": torch.cuda.get_device_name(0)}
    lines = [f"EGVM batched against serial search_batch, fc_small_r1, eps {EPS}, depth-20 scrambles, {args.reps} alternated repetitions "
             f"after a warm-up (median [min-max]); {out['device']}"]
    legs = {"sizes": sizes_leg, "parity": parity_leg}
    for leg in args.legs.split(","):
        legs[leg](model, args, out, lines)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
