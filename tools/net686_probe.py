"""
The 6x8x6 networks on every engine in ONE process on one MI355X (formula weights, tests/formula_weights.py):

    python tools/net686_probe.py [--no-search] > profiles/net686_engines.txt

  * per architecture (fc_small 6x8x6, conv) at 11 264 and 352 rows: one forward from device cubes on the live module
    (GenericNet behind the 288-wide encoder: the route of a bare network), on the fp32 chain, on the f16x3 split engine (f32s) and
    on bf16 -- the last three through `Folded(net)`;
  * the conv branch alone: rc_conv686_branch per output format against the module's pad / unfold / addmm route on the same rows,
    and the kernel's share of the conv engines' forward;
  * fc_small 6x8x6 against fc_small 20x24 on the same engine and rows: the same kernels at the same shapes, so the two must agree
    within the run's own scatter;
  * one search: MCTS, 1 024 depth-20 trees, max_states 10 000, conv -- live module against Folded on f32s and bf16, in states/s.

Every figure: 3 warm-up calls, then 9 timed with events on the launch stream around each call; median with min - max.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd"), os.path.join(ROOT, "tests")]
from formula_weights import fill  # noqa: E402
from librubiks import cube  # noqa: E402
from librubiks.cube import cube686  # noqa: E402
from librubiks.cube.device import encode  # noqa: E402
from librubiks.model import F32_SPLIT, Folded, Model, ModelConfig, make_inference_net  # noqa: E402

ROWS = (11264, 352)


def timed(fn, reps=9, warm=3):
    """(median, min, max) in microseconds of one call of fn."""
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(t):
    return f"{t[0]:9.1f} us  ({t[1]:.1f} - {t[2]:.1f})"


def forward(engine, cubes):
    if getattr(engine, "supports_cubes", False):
        return lambda: engine.forward_cubes(cubes)
    return lambda: engine(encode(engine, cubes))


def main():
    torch.cuda.set_device(0)
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; per figure: median (min - max) of 9 calls behind 3 warm-up calls")
    np.random.seed(686)
    batches = {n: cube.scramble_batch(n, 20, True)[0] for n in ROWS}
    nets = {"fc_small-686": fill(Model.create(ModelConfig(architecture="fc_small", is2024=False))).eval(),
            "conv": fill(Model.create(ModelConfig(architecture="conv", is2024=False))).eval(),
            "fc_small-20x24": fill(Model.create(ModelConfig(architecture="fc_small", is2024=True))).eval()}
    engines, medians = {}, {}
    for name, net in nets.items():
        handle = net if net.config.is2024 else Folded(net)
        engines[name] = {"fp32 chain": make_inference_net(handle, torch.float32), "f32s": make_inference_net(handle, F32_SPLIT),
                         "bf16": make_inference_net(handle, torch.bfloat16)}
        if not net.config.is2024:
            engines[name] = {"live module": make_inference_net(net, torch.float32), **engines[name]}
    print("\n== one forward from device cubes (12 logits + value per row)")
    for n in ROWS:
        for name in ("fc_small-686", "fc_small-20x24", "conv"):
            for which, eng in engines[name].items():
                t = medians[name, which, n] = timed(forward(eng, batches[n]))
                print(f"{name:15s} {which:11s} {n:6d} rows: {fmt(t)}")
    print("\n== fc_small 6x8x6 against fc_small 20x24 on the same engine (same kernels, same shapes)")
    for n in ROWS:
        for which in ("f32s", "bf16", "fp32 chain"):
            a, b = medians["fc_small-686", which, n], medians["fc_small-20x24", which, n]
            inside = "within" if a[1] <= b[2] and b[1] <= a[2] else "OUTSIDE"
            print(f"{which:11s} {n:6d} rows: 6x8x6 {a[0]:.1f} us, 20x24 {b[0]:.1f} us, ratio {a[0] / b[0]:.3f} -- {inside} the two min - max ranges")
    print("\n== the conv branch alone: rc_conv686_branch per output format, and the module's pad / unfold / addmm route on the same rows")
    conv = nets["conv"]
    branch = engines["conv"]["f32s"]._conv
    for n in ROWS:
        cubes = batches[n]
        oh = cubes.as_oh686(torch.float32)

        def live():
            y = cube686.as_correct(oh)
            from librubiks.model import _conv1d_k3
            for m in conv.shared_conv_net:
                y = _conv1d_k3(y, m) if isinstance(m, torch.nn.Conv1d) else m(y)
            return y.reshape(n, -1)
        with torch.no_grad():
            t_live = timed(live)
        print(f"module route (from the one-hot)      {n:6d} rows: {fmt(t_live)}")
        for f, (label, dtype, eng) in enumerate((("float", torch.float32, "fp32 chain"), ("bf16", torch.bfloat16, "bf16"), ("half hi|lo", torch.float16, "f32s"))):
            out = torch.empty((n, 2048 if f == 2 else 1024), dtype=dtype, device="cuda")
            t = timed(lambda: branch.launch(cubes, out, 0, f))
            whole = medians["conv", eng, n]
            print(f"rc_conv686_branch format {f} ({label:10s}) {n:6d} rows: {fmt(t)}   = {100 * t[0] / whole[0]:.1f} % of the {eng} forward ({whole[0]:.1f} us); "
                  f"module route / kernel = {t_live[0] / t[0]:.1f}")
    if "--no-search" in sys.argv:
        return
    print("\n== MCTS, 1 024 depth-20 trees, max_states 10 000, conv network (one search each behind a warm-up search of the same shape)")
    from librubiks.solving.agents import MCTS
    np.random.seed(0)
    roots = cube.scramble_batch(1024, 20, True)[0]
    base = None
    for label, net, dt in (("live module (bare network)", conv, F32_SPLIT), ("Folded, f32s", Folded(conv), F32_SPLIT), ("Folded, bf16", Folded(conv), torch.bfloat16)):
        agent = MCTS(net, c=0.6, search_graph=True, net_dtype=dt)
        agent.search_batch(roots, None, 10_000)
        res = agent.search_batch(roots, None, 10_000)
        rate = float(res.nodes.sum()) / res.seconds
        base = base or rate
        print(f"{label:28s}: {res.nodes.sum():9d} states in {res.seconds:7.3f} s = {rate / 1e6:6.2f} M states/s ({rate / base:.2f} x the live module), "
              f"solved {int(res.solved.sum())} / 1024")


if __name__ == "__main__":
    main()
