"""
The input layer of the split network both ways, same box: rc_first_layer_gather_f16 (sum of 20 fp32 rows of W^T per state) against
rc_first_layer_split_flag_f16 (one-hot MFMA, hi / lo tables), microseconds per launch as a replayed graph of `reps` launches.

    python tools/input_layer_ab.py [--form F] [--packed R] [rows ...]

--form F    the gather kernel through rc_first_layer_gather_rows_f16 with the identity map and its form forced (1: sixteen waves x four
            columns per lane, 2: twelve waves x eight columns), next to the form the library chooses by itself
--packed R  the packed entry as an MCTS step calls it: R rows exist (a device word), a map that permutes the states
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-rubiks_amd")]
from librubiks import _hip, cube  # noqa: E402
from librubiks.model import F32_SPLIT, Model, ModelConfig, make_inference_net  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--form", type=int, choices=(1, 2))
ap.add_argument("--packed", type=int)
ap.add_argument("rows", type=int, nargs="*")
args = ap.parse_args()
rows_list = args.rows or [352, 1408, 5632, 11264, 196608]
torch.manual_seed(0)
np.random.seed(0)
eng = make_inference_net(Model.create(ModelConfig(architecture="fc_small")).eval().cuda(), F32_SPLIT)


def graph_us(fn, reps=20):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
        g.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(5):
            g.replay()
        b.record(s)
        torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / (5 * reps)


def rows_entry(cubes, R, src, form):
    """The input layer of the engine's first layer through the packed entry: R of cubes.n rows, state src[r] behind row r."""
    _, _, b, code, alpha, Wh, _, Wrows = eng.layers[0][:8]
    H = Wh.shape[0]
    out = torch.empty((cubes.n, 2 * H), dtype=torch.float16, device="cuda")
    word = torch.tensor([R, 0, 0, 0], dtype=torch.int32, device="cuda")
    return lambda: _hip.check(_hip.lib().rc_first_layer_gather_rows_f16(cubes.soa.data_ptr(), cubes.n, cubes.stride, Wrows.data_ptr(), b.data_ptr(),
                                                                        out.data_ptr(), H, code, alpha, eng.range_flag.data_ptr(), word.data_ptr(),
                                                                        src.data_ptr(), form, _hip.stream_ptr()), "rc_first_layer_gather_rows_f16")


for rows in rows_list:
    cubes, _, _ = cube.scramble_batch(rows, 30, True)
    if args.packed is not None:
        R = min(args.packed, rows)
        src = torch.randperm(rows, generator=torch.Generator().manual_seed(rows)).int().cuda()
        us = {form: graph_us(rows_entry(cubes, R, src, form)) for form in ((args.form,) if args.form else (0, 1, 2))}
        print(f"rows {rows:7d}, {R:7d} packed: " + "   ".join(f"form {f}: {u:8.1f} us" for f, u in us.items()), flush=True)
        continue
    if args.form:
        ident = torch.arange(rows, dtype=torch.int32, device="cuda")
        eng.gather_input = True
        chosen = graph_us(lambda: eng._first_from_cubes(cubes, eng.layers))
        print(f"rows {rows:7d}: form {args.form} {graph_us(rows_entry(cubes, rows, ident, args.form)):8.1f} us   chosen by the library {chosen:8.1f} us", flush=True)
        continue
    out = {}
    for name, flag in (("gather", True), ("mfma", False)):
        eng.gather_input = flag
        out[name] = graph_us(lambda: eng._first_from_cubes(cubes, eng.layers))
    eng.gather_input = True
    print(f"rows {rows:7d}: gather {out['gather']:8.1f} us   one-hot MFMA {out['mfma']:8.1f} us", flush=True)
