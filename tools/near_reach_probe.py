"""
What the search beyond the near-solved table costs and what it tells, on one MI355X (NearTable.reach, csrc/rubiks_near_reach.hip,
DESIGN §3.5f).

  reach K     the table of depth K; `rc_near_depth` on 2^20 depth-20 scrambles already on the device, by HIP events (the random
              read rate that exists); then 1 024 states scrambled 12, 14, 16 and 20 moves through reach(extra=8): per level the
              states still without a distance, the seconds (sum of the launches' HIP events), the canonical sequences probed and
              their rate, the longest launch; and the share of states that have their distance at every K + J, J = 2 .. 8
  flight      reach(extra=--flight-extra) on the depth-20 states at K = 8 with the library as built (two probes of a lane in
              flight) and with --flight1-lib (make -C rl-rubiks_amd flight1: one), each in a process of its own
  egvm, sampled, mcts   tools/near_probe.py's three searches (trained weights fc_small_r1); the exact distances of their
              scrambles from reach(extra=8) at K = 8, once; the share of solved games whose distance is known (<= 16), and over
              those the mean excess (length - distance) of the queues as searched, after `shortened`, and after
              `shortened().tightened(table)` at K = 6 and K = 8

Without --leg the legs run one after the other, each as a process of its own under its own time limit; the first that fails or
runs out of time ends the run.  Every leg appends its lines to the text file.

    make -C rl-rubiks_amd flight1 && python tools/near_reach_probe.py --out profiles/near_reach_probe.txt
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd"), os.path.join(ROOT, "tools")]

SCRAMBLES = [12, 14, 16, 20]
EXTRA = 8
LEG_SECONDS = {"reach6": 240, "reach8": 420, "flight2": 180, "flight1": 180, "egvm": 300, "sampled": 300, "mcts": 300}
FLIGHT1_LIB = os.path.join(ROOT, "rl-rubiks_amd", "lib", "librubiks_hip_flight1.so")


def canonical_counts(levels: int) -> list:
    """Sequences of j = 0 .. levels moves that the device walks (near_reach_model.canonical's three rules), counted by the last
    move and whether the one before equals it."""
    once, twice, counts = np.ones(12, dtype=np.int64), np.zeros(12, dtype=np.int64), [1, 12]
    for _ in range(2, levels + 1):
        new_once, new_twice = np.zeros(12, dtype=np.int64), np.zeros(12, dtype=np.int64)
        for p in range(12):
            for a in range(12):
                if a == (p ^ 1) or ((a >> 1) == ((p >> 1) ^ 1) and (p >> 1) > (a >> 1)):
                    continue
                if a == p:
                    new_twice[a] += once[p]              # (a third equal turn is left out)
                else:
                    new_once[a] += once[p] + twice[p]
        once, twice = new_once, new_twice
        counts.append(int(once.sum() + twice.sum()))
    return counts[:levels + 1]


def event_seconds(pairs) -> list:
    return [a.elapsed_time(b) / 1e3 for a, b in pairs]


def depth_rate(table, emit):
    import ctypes
    import torch
    from librubiks import _hip, cube
    np.random.seed(2)
    cubes = cube.scramble_batch(1 << 20, 20, True)[0]
    out, status = torch.empty(1 << 20, dtype=torch.int8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    secs = []
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _hip.check(table.lib.rc_near_depth(ctypes.byref(table.struct), cubes.soa.data_ptr(), cubes.n, cubes.stride, out.data_ptr(), None,
                                           status.data_ptr(), _hip.stream_ptr()), "rc_near_depth")
        b.record()
        torch.cuda.synchronize()
        secs.append(a.elapsed_time(b) / 1e3)
    s = float(np.median(secs[1:]))
    emit(f"K={table.depth}: rc_near_depth on 2^20 depth-20 scrambles {s * 1e6:.1f} us by events = {(1 << 20) / s / 1e9:.2f} G probes/s")


def reach_lines(table, states, tag, emit, extra=EXTRA):
    """One reach(extra) with the launches timed; -> the result."""
    import torch
    from librubiks.solving import near
    counts = canonical_counts(extra)
    timings = {}
    torch.cuda.synchronize()
    res = table.reach(states, extra=extra, timings=timings)
    torch.cuda.synchronize()
    n, K = len(res.distances), table.depth
    P = near.default_prefix(n, extra)
    live = n - int((res.levels == 0).sum())
    total, longest = 0.0, 0.0
    for level in sorted(timings):
        secs = event_seconds(timings[level])
        leaves = live * counts[level]
        emit(f"{tag} level {level}: {live} states, {len(secs)} launches, {sum(secs):.4f} s = {sum(secs) / live * 1e3:.4f} ms a state, "
             f"{leaves:.3e} sequences = {leaves / sum(secs) / 1e9:.2f} G probes/s, longest launch {max(secs):.4f} s "
             f"({near.default_launch_items(level, P)} items of 12^{level - min(level, P)} a launch)")
        total, longest = total + sum(secs), max(longest, max(secs))
        live -= int((res.levels == level).sum())
    shares = ", ".join(f"{K + J}: {np.mean((res.levels >= 0) & (res.levels <= J)):.4f}" for J in range(2, extra + 1))
    emit(f"{tag}: {n} states, prefix {P}, {total:.3f} s in the levels' launches, {res.seconds:.3f} s wall = {res.seconds / n * 1e3:.3f} ms a state; "
         f"longest launch {longest:.4f} s; share with a distance by K + J: {shares}; mean distance of those {res.distances[res.distances >= 0].mean():.2f}")
    return res


def leg_reach(K, emit):
    import torch
    from librubiks import cube
    from librubiks.solving.near import NearTable
    emit(f"device: {torch.cuda.get_device_name(0)}")
    table = NearTable(K)
    depth_rate(table, emit)
    for moves in SCRAMBLES:
        np.random.seed(moves)
        states = cube.scramble_batch(1024, moves, True)[0]
        reach_lines(table, states, f"K={K} scrambled {moves}", emit)


def leg_flight(name, args, emit):
    from librubiks import _hip, cube
    from librubiks.solving.near import NearTable
    np.random.seed(20)
    states = cube.scramble_batch(1024, 20, True)[0]
    table = NearTable(8)
    table.reach(states, extra=4)                                                            # warm-up
    reach_lines(table, states, f"{name} ({os.path.basename(_hip.LIB_PATH)}) K=8 scrambled 20", emit, extra=args.flight_extra)


def leg_agent(name, emit):
    import torch
    from librubiks import cube
    from librubiks.model import F32_SPLIT, Model
    from librubiks.solving.agents import EGVM, MCTS, PolicySearch
    from librubiks.solving.near import NearTable
    from near_probe import D, DEPTHS, EPS, W
    model = Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).cuda().eval()
    if name == "sampled":
        from rollout_batch_probe import pooled, scrambles
        states = pooled(scrambles(500, DEPTHS))
        raw = PolicySearch(model, sample_policy=True, net_dtype=F32_SPLIT).search_batch(states, None, 200, seeds=1)
    else:
        np.random.seed(1)
        states = cube.scramble_batch(1024, 20, True)[0]
        seeds = np.random.randint(0, 2 ** 31 - 1, 1024)
        if name == "egvm":
            raw = EGVM(model, EPS, W, D, net_dtype=F32_SPLIT).search_batch(states, None, 50_000, seeds=seeds)
        else:
            raw = MCTS(model, c=0.6, search_graph=True, net_dtype=F32_SPLIT).search_batch(states, None, 175_000)
    won = np.flatnonzero(np.asarray(raw.solved, dtype=bool))
    rows = states.numpy() if hasattr(states, "soa") else np.asarray(states)
    short = raw.shortened(states)
    variants = [("as searched", raw), ("shortened", short)]
    for K in (6, 8):
        variants.append((f"shortened, tightened K={K}", short.tightened(NearTable.get(K))))
    table = NearTable.get(8)
    t0 = time.perf_counter()
    dist = table.reach(rows[won], extra=EXTRA).distances.astype(np.int64)
    dt = time.perf_counter() - t0
    known = dist >= 0
    emit(f"{name}: {len(raw.solved)} games, {len(won)} solved; exact distances of the solved games' scrambles by reach(extra={EXTRA}) at K=8 in {dt:.2f} s: "
         f"{int(known.sum())} known (<= {8 + EXTRA}) = {known.mean():.4f}, mean distance of those {dist[known].mean() if known.any() else float('nan'):.2f}")
    for what, res in variants:
        lengths = np.asarray(res.lengths)[won].astype(np.int64)
        excess = (lengths - dist)[known]
        assert (excess >= 0).all()
        emit(f"{name} {what}: mean length {lengths.mean():.2f} over all solved; over the {int(known.sum())} with a known distance: mean length "
             f"{lengths[known].mean():.2f}, mean excess {excess.mean():.2f}, optimal {np.mean(excess == 0):.4f}")
    if name == "sampled":                                                                   # the public call gives the same numbers
        again = variants[-1][1].excess(table, states, extra=EXTRA)
        assert np.array_equal(again[won][known], (np.asarray(variants[-1][1].lengths)[won] - dist)[known]) and (again[won][~known] == -1).all()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/near_reach_probe.txt")
    ap.add_argument("--leg", default=None, help=", ".join(LEG_SECONDS) + " (default: all, a process each)")
    ap.add_argument("--flight-extra", type=int, default=7)
    ap.add_argument("--flight1-lib", default=FLIGHT1_LIB)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.leg is None:
        with open(args.out, "w") as f:
            f.write("search beyond the near-solved table: NearTable.reach, 1 024 states a batch; launch seconds by HIP events\n"
                    "(python tools/near_reach_probe.py; one process per leg, each under its own time limit: " + ", ".join(LEG_SECONDS) + ")\n")
        for leg, limit in LEG_SECONDS.items():
            env = dict(os.environ)
            if leg == "flight1":
                if not os.path.exists(args.flight1_lib):
                    with open(args.out, "a") as f:
                        f.write(f"flight1: {args.flight1_lib} is not built (make -C rl-rubiks_amd flight1): leg left out\n")
                    continue
                env["RUBIKS_HIP_LIB"] = args.flight1_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--leg", leg, "--flight-extra", str(args.flight_extra)]
            try:
                rc = subprocess.run(cmd, timeout=limit, env=env).returncode
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
    if args.leg.startswith("reach"):
        leg_reach(int(args.leg[5:]), emit)
    elif args.leg.startswith("flight"):
        leg_flight(args.leg, args, emit)
    else:
        leg_agent(args.leg, emit)


if __name__ == "__main__":
    main()
