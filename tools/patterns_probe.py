"""
What mining generalised patterns costs on the device (librubiks/analysis/pattern_mining.py, csrc/rubiks_patterns.hip) beside the
plain Python restatement of the reference's rules (`mine_plain` in tests/patterns_model.py), on one MI355X, trained weights
fc_small_r1, support 0.3:

  astar_1k     the reference's run: 1 000 A* games (lambda 0.16, N 700) on scrambles of 100 .. 999 moves (`generate_actions`)
  astar_many   --many such games (default 100 000) as one pool of --slots slots, bounded by --many-seconds of search
  egvm_short   1 024 EGVM games at api.py's parameters (eps 0.375, W 10, D 50; depth-20 scrambles, max_states 50 000), shorten=True
  egvm_walk    the same games as the walks the agent returns without it

Per case: games, solved, moves in all, mean and longest solution; wall seconds of find_generalized_patterns on the solved games'
queues (upload, every level's launches and read-backs, the dict; --reps runs after a warm-up, median [min-max]), the levels it
ran and the patterns it found; wall seconds of mine_plain on the first --plain sequences (all of astar_1k) and, labelled as one,
the extrapolation to the whole case by moves^3 (the restatement's cost per sequence is cubic in its length).  Where mine_plain
ran on the whole case its result is compared with the device's.

    python tools/patterns_probe.py --out profiles/patterns_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd"), os.path.join(ROOT, "tests")]

SUPPORT = 0.3
EPS, W, D = 0.375, 10, 50


def measure(name, table, solved, args, lines):
    """table: the QueueTable of a search; solved: bool per game."""
    import patterns_model as pm
    from librubiks.analysis import pattern_mining as mining
    idx = np.flatnonzero(solved)
    acts, lens = table.padded(idx, fill=0)
    if len(idx) == 0:
        lines.append(f"{name:11s} games {len(solved)} solved 0: nothing to mine")
        return
    form = (acts if acts.shape[1] else np.zeros((len(idx), 1), dtype=np.uint8), lens)
    secs = []
    for rep in range(args.reps + 1):   # rep 0: warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        found = mining.find_generalized_patterns(form, SUPPORT)
        secs.append(time.perf_counter() - t)
    secs = sorted(secs[1:])
    batch = mining.PatternBatch(form[0], lens, mining.min_count(len(idx), SUPPORT))
    batch.run()
    levels = int(batch.struct.level)
    k = len(idx) if name == "astar_1k" else min(args.plain, len(idx))
    t = time.perf_counter()
    plain = pm.mine_plain([acts[s, :lens[s]].tolist() for s in range(k)], SUPPORT)
    plain_s = time.perf_counter() - t
    cube_all, cube_k = float((lens.astype(np.float64) ** 3).sum()), float((lens[:k].astype(np.float64) ** 3).sum())
    lines.append(f"{name:11s} games {len(solved)} solved {len(idx)}  moves {int(lens.sum())}  mean {lens.mean():.1f}  longest {int(lens.max())}  "
                 f"workspace {mining.workspace_bytes(int(lens.sum())) / 2 ** 20:.1f} MiB")
    lines.append(f"{'':11s} device: {np.median(secs):.4f} s [{secs[0]:.4f}-{secs[-1]:.4f}], levels up to {levels}, {len(found)} patterns, "
                 f"first {list(found.items())[:3]}")
    if k == len(idx):
        same = list(plain.items()) == list(found.items())
        lines.append(f"{'':11s} mine_plain on all {k}: {plain_s:.2f} s, result {'equal to' if same else 'DIFFERENT from'} the device's; "
                     f"plain / device = {plain_s / np.median(secs):.1f}")
    else:
        lines.append(f"{'':11s} mine_plain on the first {k} sequences ({int(lens[:k].sum())} moves): {plain_s:.2f} s; EXTRAPOLATED by moves^3 "
                     f"to all {len(idx)}: {plain_s * cube_all / max(cube_k, 1.0):.1f} s (not measured)")
    print("\n".join(lines[-3:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/patterns_probe.txt")
    ap.add_argument("--cases", default="astar_1k,egvm_short,egvm_walk,astar_many")
    ap.add_argument("--many", type=int, default=100_000)
    ap.add_argument("--many-seconds", type=float, default=240.0)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--max-states", type=int, default=175_000)   # (at 50 000 -- six iterations of N 700 -- A* solved none of these scrambles)
    ap.add_argument("--plain", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from librubiks import cube
    from librubiks.model import Model
    from librubiks.solving.agents import EGVM, AStar
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    lines = [f"find_generalized_patterns at support {SUPPORT} beside mine_plain; fc_small_r1, bf16 engine; {args.reps} runs after a warm-up "
             f"(median [min-max]); A* max_states {args.max_states}, {args.slots} slots; {torch.cuda.get_device_name(0)}"]
    for name in args.cases.split(","):
        t = time.perf_counter()
        if name.startswith("astar"):
            games = 1000 if name == "astar_1k" else args.many
            np.random.seed(0)
            states = cube.scramble_batch(games, lambda: np.random.randint(100, 1000), True)[0]
            agent = AStar(model, 0.16, 700, net_dtype=torch.bfloat16)
            res = agent.search_batch(states, None if name == "astar_1k" else args.many_seconds, args.max_states, slots=args.slots)
        else:
            np.random.seed(1)
            states = cube.scramble_batch(1024, 20, True)[0]
            seeds = np.random.randint(0, 2 ** 31 - 1, 1024)
            agent = EGVM(model, EPS, W, D, net_dtype=torch.bfloat16, shorten=name == "egvm_short")
            res = agent.search_batch(states, None, 50_000, seeds=seeds)
        torch.cuda.synchronize()
        lines.append(f"{name:11s} search {time.perf_counter() - t:.1f} s (scrambles included)")
        measure(name, res.queues, np.asarray(res.solved, dtype=bool) & (res.queues.lengths() > 0), args, lines)
        del agent, res
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
