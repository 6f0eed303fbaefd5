"""bench.py without --full: the headline alone (set-up, warm-up, timed steps, --dump-outputs, one line), none of the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "towers_ab", "flip_rate_vs_f32", "f32_mode", "fp8_mode", "map_eval", "loss_fwd", "train_step",
             "input_pipeline", "code_loop", "map_eval_nuswide", "twdh_fp8", "mith_step", "dchmt_epoch", "cpu_baseline")


def test_plain_run_is_the_headline_alone(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CMH_FORCE_DIST")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, res.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["unit"] == "pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["value"] > 0 and abs(rec["value"] - 2 * 256 / (rec["ms_per_step"] * 2e-3)) < 1e-3 * rec["value"]
    assert rec["value_dense_text"] is None
    assert not [k for k in FULL_ONLY if k in rec], rec.keys()
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["image_codes", "image_hash", "loss", "text_codes", "text_hash"]
    assert got["image_hash"].shape == (256, 64) and got["text_codes"].shape == (256, 64) and np.isfinite(got["loss"]).all()
