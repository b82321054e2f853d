"""
bench.py without --full: the headline leg's prep, warm-up and exactly --steps timed steps, and nothing behind them -- no spread
windows, pool tail, run to completion, phases, other legs, extra legs, roofline_env or cpu_baseline.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_is_the_headline_window(tmp_path):
    detail = tmp_path / "detail.json"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--trees", "48",
           "--pool-factor", "2", "--solve-max-states", "1500", "--prep-cap", "40", "--detail", str(detail)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    with open(detail) as f:
        full = json.load(f)
    assert line["steps"] == 7 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["dtype"].startswith("f32 (f16x3 split") and line["value"] == full["legs"]["f32s"]["value"]
    assert list(full["legs"]) == ["f32s"]
    leg = full["legs"]["f32s"]
    assert leg["steps_timed"] == 7 and leg["value_spread"] is None
    for moved in ("pool_run", "run_to_completion", "phases_ms", "roofline"):
        assert moved not in leg, moved
    for moved in ("astar", "adi", "config5_share", "roofline_env", "cpu_baseline"):
        assert moved not in full, moved
    assert full["efficiency"] is None and full["config"]["results"]["value_run_to_completion"] is None
