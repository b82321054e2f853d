"""
The 6x8x6 kernels against their 20x24 counterparts in ONE run on one MI355X: achieved algorithmic bytes per second and the share of
the HBM peak, at the sizes tools/env_bench.py uses (2^24 states for multi_rotate, 2^20 for the one-hot encoders).

    python tools/env686_probe.py [log2 n] > profiles/env686_probe.txt

The yardstick is the share of peak rc_multi_rotate and rc_as_oh_f32 reach in the same process.  Per kernel: 3 warm-up launches,
then 20 timed with events around each; median and best are reported (the clocks and the allocator have settled after the
warm-up, and the median is robust against a neighbour's burst on a shared machine).  The kernels are interleaved in two passes
(A B C ... A B C ...) so a drift of the machine shows as a difference between the passes, not between the kernels.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd")]
from librubiks.cube import DeviceCubes, DeviceCubes686  # noqa: E402

HBM_PEAK = 8000.0  # GB/s, as tools/env_bench.py


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return ts[len(ts) // 2] * 1e-3, ts[0] * 1e-3


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    n = 1 << logn
    g = torch.Generator(device="cuda").manual_seed(0)
    cubes = DeviceCubes.solved(n)
    for _ in range(30):
        cubes = cubes.multi_rotate(torch.randint(0, 12, (n,), dtype=torch.uint8, device="cuda", generator=g))
    act = torch.randint(0, 12, (n,), dtype=torch.uint8, device="cuda", generator=g)
    out20, cubes686, out686 = DeviceCubes.empty(n), cubes.to686(), DeviceCubes686.empty(n)
    no = n // 16
    small20 = DeviceCubes(cubes.soa[:, :max(256, no)].contiguous(), no)
    small686 = DeviceCubes686(cubes686.soa[:, :max(256, no)].contiguous(), no)
    oh480 = torch.empty((no, 480), dtype=torch.float32, device="cuda")
    oh288 = torch.empty((no, 288), dtype=torch.float32, device="cuda")
    # (name, algorithmic bytes per state, states, launch): bytes = planes read + action byte + planes written / row written
    kernels = [("rc_multi_rotate", 41, n, lambda: cubes.multi_rotate(act, out=out20)),
               ("rc686_multi_rotate", 97, n, lambda: cubes686.multi_rotate(act, out=out686)),
               ("rc_as_oh_f32", 20 + 1920, no, lambda: small20.as_oh(out=oh480)),
               ("rc686_as_oh_f32", 48 + 1152, no, lambda: small686.as_oh(out=oh288)),
               ("rc_as_oh686_from2024_f32", 20 + 1152, no, lambda: small20.as_oh686(out=oh288))]
    res = {"device": torch.cuda.get_device_name(0), "log2_n": logn, "hbm_peak_GBps": HBM_PEAK, "passes": []}
    for _ in range(2):
        rows = {}
        for name, unit_bytes, units, fn in kernels:
            med, best = timed(fn)
            rows[name] = {"states": units, "bytes_per_state": unit_bytes, "ms_median": round(med * 1e3, 4), "ms_best": round(best * 1e3, 4),
                          "GBps": round(unit_bytes * units / med / 1e9, 1), "frac_of_peak": round(unit_bytes * units / med / 1e9 / HBM_PEAK, 4),
                          "Mstates_per_s": round(units / med / 1e6, 1)}
        res["passes"].append(rows)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
