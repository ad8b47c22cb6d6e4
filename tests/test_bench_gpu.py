"""bench.py's command line on one GPU: a plain run reports the timed steps only, --dump-outputs writes what the
last timed step left, and the same arguments give the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARENAS, T, STEPS = 64, 16, 2


def _bench(*extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "0", "--arenas", str(ARENAS),
           "--rollout", str(T), "--mesh", "synthetic", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dump(gpu, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _bench("--dump-outputs", a)
    _bench("--dump-outputs", b)
    assert out["steps"] == STEPS and out["unit"] == "env-steps/s" and out["higher_is_better"] is True
    want = ARENAS * T * STEPS / (out["ms_per_step"] * STEPS / 1e3)
    assert abs(out["value"] - want) <= 1e-6 * want, (out["value"], want)
    assert out["roofline"]["units_per_launch"] == ARENAS
    for k in ("learn_roofline", "gae_micro", "legs", "cpu_baseline"):  # these take runs of their own: --full
        assert k not in out, k
    P = 4 * ARENAS
    shapes = {"obs": (T + 1, P, 167), "masks": (T + 1, P, 90), "actions": (T, P), "logp": (T, P), "rewards": (T, P),
              "terms": (T, P), "values": (T + 1, P), "adv": (T, P), "target": (T, P), "ret": (T, P)}
    names = sorted(f[:-4] for f in os.listdir(a))
    assert names == sorted(list(shapes) + ["params"])
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n + ".npy")), np.load(os.path.join(b, n + ".npy"))
        total += x.nbytes
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        if n in shapes:  # below the sampling threshold an array keeps its shape
            assert x.shape == shapes[n] or x.shape == (1 << 20,), (n, x.shape)
        assert np.array_equal(x, y), n  # fixed seeds: identical inputs, identical outputs
    assert total <= 64 << 20
    m = np.load(os.path.join(a, "masks.npy"))
    act = np.load(os.path.join(a, "actions.npy")).astype(np.int64)
    # the stored actions are valid ones (a finished iteration leaves the next rollout's start in row 0)
    assert np.take_along_axis(m[1:T], act[1:, :, None], axis=2).min() == 1
