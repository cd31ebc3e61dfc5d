"""bench.py's two modes: a plain run measures and reports the headline figure only; --full adds, after the timed region, what the
headline does not need (roofline pass, argmax contract, soak).  The timed step and what --dump-outputs writes are the same in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2"] + list(flags),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_reports_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-cpu-baseline", "--soak-seconds", "0.2", "--dump-outputs", str(tmp_path / "full"))
    for out in (plain, full):
        assert all(k in out for k in HEADLINE_KEYS), out
        assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert out["ms_per_step"] > 0 and out["value"] > 0
    assert "roofline" not in plain and "cpu_baseline" not in plain, plain
    assert plain["config"]["soak"] is None and "argmax_contract" not in plain["config"], plain["config"]
    assert full["roofline"]["launches"] > 0 and full["roofline"]["achieved"] > 0, full.get("roofline")
    assert full["config"]["soak"]["steps"] >= 1 and "argmax_contract" in full["config"], full["config"]
    assert "cpu_baseline" not in full                       # --no-cpu-baseline still takes it away
    # the extra work runs after the timed region and the dump: the same step, the same bits
    assert plain["config"]["final_loss"] == full["config"]["final_loss"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype == b.dtype and np.array_equal(a, b), n
