"""bench.py without --full (the headline line alone) and its --dump-outputs: what the timed steps returned, as .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_line_and_dump(tmp_path):
    """The same five steps split two ways, W = 2 + K = 3 and W = 1 + K = 4: each run prints one plain line and dumps the losses of
    exactly its K timed steps, the last of which is loss.npy.  Same seed, same trajectory: the three steps both runs time agree to the
    float atomics' rounding (graph replay vs eager agree to 1e-5 over the first steps)."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    timed = {}
    for warmup, steps in ((2, 3), (1, 4)):
        d = tmp_path / ("w%d" % warmup)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", str(steps),
                            "--warmup", str(warmup), "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        r = json.loads(lines[0])
        assert r["steps"] == steps and r["warmup"] == warmup and r["n_gpus"] == 1 and r["unit"] == "views/s" and r["dtype"] == "f32"
        assert r["higher_is_better"] and r["value"] > 0 and abs(r["value"] - 1e3 / r["ms_per_step"]) <= 1e-2 * r["value"]
        assert not {"roofline", "twin", "drift", "cpu_baseline", "concurrent_views", "note"} & set(r)   # side measurements: --full only
        assert sorted(os.listdir(d)) == ["loss.npy", "timed_losses.npy"]
        loss, tl = np.load(d / "loss.npy"), np.load(d / "timed_losses.npy")
        assert loss.dtype == tl.dtype == np.float32 and loss.shape == (1,) and tl.shape == (steps,)
        assert np.isfinite(tl).all() and (tl > 0).all() and loss[0] == tl[-1]
        timed[warmup] = tl
    a, b = timed[2], timed[1][1:]
    assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (a, timed[1])
    assert timed[1][0] != a[0]   # the extra timed step of the second run renders another view
