"""bench.py on the GPU: a plain run does only the timed path (no leg of --full in its line) and --dump-outputs writes what the
last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert abs(j["value"] - 32 * 1e3 / j["ms_per_step"]) < 0.01 * j["value"]
    assert (j["unit"], j["higher_is_better"], j["dtype"]) == ("images/s", True, "bf16")
    for leg in ("roofline", "roofline_gemm", "roofline_vq_decode", "other_configs", "cpu_baseline",
                "images_per_s_with_one_chain_in_flight", "images_per_s_with_one_step_in_flight"):
        assert leg not in j, leg
    imgs, toks = np.load(out / "images.npy"), np.load(out / "tokens.npy")
    assert imgs.dtype == toks.dtype == np.float32
    assert imgs.shape == (32, 384, 384, 3) and toks.shape == (32, 576)
    assert np.array_equal(imgs, np.round(imgs)) and imgs.min() >= 0 and imgs.max() <= 255 and 8 < imgs.std() < 128
    assert np.array_equal(toks, np.round(toks)) and toks.min() >= 0 and toks.max() < 16384
