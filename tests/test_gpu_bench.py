"""GPU: a plain `bench.py --gpus 1` run -- the headline line alone (no side measurements without --full), the step count it was
given, and the outputs --dump-outputs writes after the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["ms_per_step"] > 0 and d["value"] > 0
    for key in ("side", "roofline", "cpu_baseline"):
        assert key not in d, key
    losses, params, grads = (np.load(out / (n + ".npy")) for n in ("losses", "params", "grads"))
    assert losses.dtype == params.dtype == grads.dtype == np.float32
    from sdumc_amd import engine
    lay = engine.ParamLayout.get(*d["config"]["feature_dims"][:3])
    assert losses.shape == (8,) and params.size == lay.total == d["config"]["param_buffer_floats"] and grads.size == lay.live
    assert np.isfinite(losses[:7]).all() and np.isfinite(params).all() and np.isfinite(grads).all()
    assert round(float(losses[0]), 5) == d["config"]["final_loss"]
    assert losses.nbytes + params.nbytes + grads.nbytes <= 64 << 20
