"""
What the near-solved table costs and what tightening brings, on one MI355X, trained weights fc_small_r1 (librubiks/solving/near.py,
csrc/rubiks_near.hip).

  table K     build seconds (first build of the process and the median of --reps more), nodes and bytes of the table of depth K,
              and `depths` on 2^20 depth-20 scrambles already on the device (median of --reps calls after a warm-up)
  egvm        api.py's EGVM parameters (eps 0.375, W 10, D 50) on 1 024 depth-20 scrambles at max_states 50 000, f32s, lock step
  sampled     PolicySearch(sample_policy=True) on the evaluation protocol's 2 500 games at max_states 200  (both as
              tools/shorten_probe.py runs them)
  mcts        config #2: MCTS(c 0.6, search_graph=True) on 1 024 depth-20 scrambles at max_states 175 000, f32s
  For each of the three: mean length of the solved games' queues as searched, after `shortened`, and after
  `shortened().tightened(table, window)` for every K and window, the share of solved games the tightening made shorter, and the
  wall seconds of `tightened` (median of --reps calls after a warm-up).

Without --leg the legs run one after the other, each as a process of its own under its own time limit; the first that fails or
runs out of time ends the run.  Every leg appends its lines to the text file.

    python tools/near_probe.py --out profiles/near_table_probe.txt
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd")]

EPS, W, D = 0.375, 10, 50
DEPTHS = [10, 15, 20, 25, 30]
WINDOWS = [32, 128, None]
LEG_SECONDS = {"table": 240, "egvm": 300, "sampled": 240, "mcts": 300}


def med(xs):
    xs = sorted(float(x) for x in xs)
    return f"{np.median(xs):.4f} [{xs[0]:.4f}-{xs[-1]:.4f}]"


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, res


def leg_table(args, emit):
    import torch
    from librubiks import cube
    from librubiks.solving.near import NearTable
    np.random.seed(2)
    states = cube.scramble_batch(1 << 20, 20, True)[0]
    for K in args.depths:
        first, table = timed(lambda: NearTable(K))
        again, device_ms = [], []
        for _ in range(args.reps):
            del table
            torch.cuda.empty_cache()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dt, table = timed(lambda: NearTable(K))
            b.record()
            torch.cuda.synchronize()
            again.append(dt)
            device_ms.append(a.elapsed_time(b) / 1e3)         # the same window by HIP events on the build's stream
        rows = 12 * int(table.counts[:-1].sum())                # child rows the build expands
        table.depths(states)
        secs = [timed(lambda: table.depths(states))[0] for _ in range(args.reps)]
        d = table.depths(states)
        emit(f"table K={K}: {table.n_nodes} nodes, {table.bytes / 2 ** 20:.1f} MiB; build {first:.4f} s first, then {med(again)} s "
             f"(by events {med(device_ms)} s; {rows} child rows = {rows / np.median(again) / 1e9:.2f} G rows/s); "
             f"depths of 2^20 depth-20 scrambles {med(secs)} s = {(1 << 20) / np.median(secs) / 1e6:.1f} M states/s with the read-back, "
             f"{int((d >= 0).sum())} of them within K")
        del table
        torch.cuda.empty_cache()


def leg_tighten(name, args, emit):
    import torch
    from librubiks import cube
    from librubiks.model import F32_SPLIT, Model
    from librubiks.solving.agents import EGVM, MCTS, PolicySearch
    from librubiks.solving.near import NearTable
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    if name == "sampled":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from rollout_batch_probe import pooled, scrambles
        states = pooled(scrambles(500, DEPTHS))
        search = lambda: PolicySearch(model, sample_policy=True, net_dtype=F32_SPLIT).search_batch(states, None, 200, seeds=1)   # noqa: E731
    else:
        np.random.seed(1)
        states = cube.scramble_batch(1024, 20, True)[0]
        seeds = np.random.randint(0, 2 ** 31 - 1, 1024)
        if name == "egvm":
            search = lambda: EGVM(model, EPS, W, D, net_dtype=F32_SPLIT).search_batch(states, None, 50_000, seeds=seeds)   # noqa: E731
        else:
            search = lambda: MCTS(model, c=0.6, search_graph=True, net_dtype=F32_SPLIT).search_batch(states, None, 175_000)   # noqa: E731
    dt, raw = timed(search)
    won = np.asarray(raw.solved, dtype=bool) & (raw.lengths > 0)
    if not won.any():
        emit(f"{name}: {len(raw.solved)} games, none solved with moves: nothing to tighten")
        return
    dt_short, short = timed(lambda: raw.shortened(states))
    emit(f"{name}: {len(raw.solved)} games, {int(won.sum())} solved with moves, search {dt:.3f} s; mean length {raw.lengths[won].mean():.2f} as searched, "
         f"{short.lengths[won].mean():.2f} after shortened() ({dt_short:.4f} s), longest {int(short.lengths[won].max())}")
    for K in args.depths:
        table = NearTable.get(K)
        for window in WINDOWS:
            short.tightened(table, window)
            runs = [timed(lambda: short.tightened(table, window)) for _ in range(args.reps)]
            tight = runs[-1][1]
            assert (tight.lengths[won] <= short.lengths[won]).all()
            emit(f"{name} K={K} window {'whole' if window is None else window}: mean {tight.lengths[won].mean():.2f}, "
                 f"{np.mean(tight.lengths[won] < short.lengths[won]):.4f} of the solved games shorter, tightened() {med([r[0] for r in runs])} s")
        NearTable._cache.clear()
        del table
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/near_table_probe.txt")
    ap.add_argument("--leg", default=None, help="table, egvm, sampled or mcts (default: all, a process each)")
    ap.add_argument("--depths", type=lambda s: [int(k) for k in s.split(",")], default=[5, 6, 7, 8])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.leg is None:
        with open(args.out, "w") as f:
            f.write(f"near-solved table: build, probe and tightening; fc_small_r1, {args.reps} runs after a warm-up (median [min-max])\n")
        for leg, limit in LEG_SECONDS.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--leg", leg, "--depths", ",".join(map(str, args.depths)),
                   "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                with open(args.out, "a") as f:
                    f.write(f"leg {leg} ended with status {rc}: the legs after it were not run\n")
                sys.exit(rc)
        return

    def emit(line):
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.leg == "table":
        import torch
        emit(f"device: {torch.cuda.get_device_name(0)}")
        leg_table(args, emit)
    else:
        leg_tighten(args.leg, args, emit)


if __name__ == "__main__":
    main()
