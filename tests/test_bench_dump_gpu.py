"""
bench.py --dump-outputs: what the timed window computed, written as .npy files after exactly --steps timed steps.  Two runs
with the same arguments see the same seeded inputs and must write the same arrays, bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--trees", "48", "--pool-factor", "2", "--legs", "f32s,bf16:window",
        "--solve-max-states", "1500", "--phase-reps", "0", "--no-cpu-baseline", "--no-env-roofline", "--prep-cap", "40",
        "--extra-legs", "none", "--window-only"]


def _run(tmp_path, tag):
    out_dir = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--detail", str(tmp_path / f"{tag}_detail.json"),
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    with open(tmp_path / f"{tag}_detail.json") as f:
        full = json.load(f)
    return line, full, {p[:-4]: np.load(out_dir / p) for p in sorted(os.listdir(out_dir))}


def test_dump_outputs_are_the_window_and_repeat_exactly(tmp_path):
    line, full, a = _run(tmp_path, "a")
    assert line["steps"] == 7 and line["ms_per_step"] > 0
    for leg in ("f32s", "bf16"):
        assert full["legs"][leg]["steps_timed"] == 7
    names = {"tree_status", "tree_nodes", "tree_iterations", "tree_path_len", "slot_game", "node_N", "node_W", "node_P", "node_V",
             "net_probs", "net_values"}
    assert set(a) == {f"{leg}_{n}" for leg in ("f32s", "bf16") for n in names}
    assert sum(x.nbytes for x in a.values()) < 64 << 20
    for key, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), key
    for leg in ("f32s", "bf16"):
        assert a[f"{leg}_tree_status"].shape == (48,) and a[f"{leg}_node_N"].shape == (48, 32, 12)
        assert a[f"{leg}_net_probs"].shape == (11 * 48, 12)
        assert (a[f"{leg}_tree_nodes"] > 0).all() and (a[f"{leg}_tree_iterations"] > 0).all()
        root_visits = a[f"{leg}_node_N"][:, 1]      # node 1 is the root (row 0 is the tree's null row)
        assert not np.isnan(root_visits).any() and (root_visits.sum(1) > 0).any()
    _, _, b = _run(tmp_path, "b")
    assert set(b) == set(a)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
