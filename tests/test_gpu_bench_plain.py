"""`python bench.py --gpus 1` without --full: the headline line only (no `parts`, no rooflines, no CPU baseline), --steps timed
steps, and --dump-outputs writing what the last timed step returned (the chain's enhanced 60 s stereo) as float32."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_prints_headline_and_dumps_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "EGREGORA_BENCH_ONE_GPU")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--iters", "40",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["higher_is_better"] is True
    assert out["unit"] == "audio-sec/sec" and out["value"] > 0 and out["ms_per_step"] > 0 and out["dtype"].startswith("f32")
    assert abs(out["value"] - 60.0 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert not {"parts", "roofline", "cpu_baseline"} & set(out)
    y = np.load(tmp_path / "fatllama_output.npy")
    assert y.dtype == np.float32 and y.shape == (2, 60 * 48000)
    assert np.isfinite(y).all() and 0 < np.abs(y).max() <= 1.0
