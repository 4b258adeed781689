"""bench.py command line on the GPU: a plain run carries only the headline
fields and skips the legs that take runs of their own; --full brings them
back; --dump-outputs writes the last timed step's verdicts, identical from
run to run (seeded inputs).  Tiny batch: this checks the plumbing, not the
figure."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu


def _gpu_available():
    try:
        from harmony_amd import core
        return core.device_count() > 0
    except Exception:
        return False


if not os.environ.get("HBLS_FORCE_GPU_TESTS"):
    pytestmark = [pytest.mark.gpu,
                  pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]

BATCH = 96
HEADLINE = {"metric": "BLS12-381 aggregate-verifies/sec (committee=4096)",
            "unit": "aggregate-verifies/sec", "higher_is_better": True,
            "dtype": "u64"}


def _bench(*extra):
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--batch", str(BATCH), *extra],
        capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout     # exactly one JSON result line
    return json.loads(lines[0])


def test_plain_run_headline_and_dump(oracle_lib, tmp_path):
    import numpy as np
    out = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k, v in HEADLINE.items():
        assert out[k] == v
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    # value and ms_per_step state the same measurement
    assert out["value"] == pytest.approx(BATCH / (out["ms_per_step"] * 1e-3), rel=1e-3)
    # legs with runs of their own stay out of a plain run
    assert out["roofline"] is None and out["cpu_baseline"] is None
    res = np.load(tmp_path / "verify_results.npy")
    assert res.dtype == np.float32 and res.shape == (BATCH,)
    assert (res == 1).all()              # every seeded item verifies
    assert sorted(os.listdir(tmp_path)) == ["verify_results.npy"]


def test_full_run_brings_roofline_back(oracle_lib):
    out = _bench("--steps", "2", "--warmup", "1", "--full", "--skip-cpu-baseline")
    for k, v in HEADLINE.items():
        assert out[k] == v
    assert out["steps"] == 2
    roof = out["roofline"]
    assert roof["bound"] == "valu" and roof["peak"] > 0
    assert set(roof["stages_ms_per_launch"]) == {
        "mask_aggregate", "hash_to_g2", "g2_decompress", "verify_pairing"}
    assert out["cpu_baseline"] is None   # --skip-cpu-baseline
