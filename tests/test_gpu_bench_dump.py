"""bench.py on the device, at a four-matrix batch as two interleaved parts (the case in which --full
adds the one-part roofline step): a plain run ends with the timed steps (none of the
--full fields) and --dump-outputs writes the last timed step's results; --full brings the parity,
API-path and one-part roofline fields back.  One fresh process per run, as the benchmark is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("parity_timed_step", "frob_err_vs_ref_sketch", "cpu_baseline", "api_path", "api_single", "roofline_solo")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "4", "--streams", "2",
                        "--steps", "1", "--warmup", "0", *args], capture_output=True, text=True, timeout=200, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0])


def test_plain_run_dumps_last_step(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert d["steps"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "matrices/s"
    assert abs(d["value"] - 4 * 1000.0 / d["ms_per_step"]) <= 1e-9 * d["value"]
    assert d["solver"]["parts"] == 2 and "concurrency" in d["roofline"]
    assert not [k for k in FULL_ONLY if k in d]
    a = {f[:-4]: np.load(os.path.join(tmp_path, f), allow_pickle=False) for f in os.listdir(tmp_path)}
    assert set(a) == {"Q", "L", "R", "Q_scale", "global_scale", "errors_Q", "errors_LR"}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k, x in a.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), k
    # L and R fit their share whole; Q (4096 x 4096) is sampled, its entries on the 2-bit grid
    assert a["L"].shape == (4, 4096, 128) and a["R"].shape == (4, 128, 4096)
    assert a["Q"].ndim == 2 and a["Q"].shape[0] == 4 and a["Q"].shape[1] < 4096 * 4096
    assert a["errors_Q"].shape == (4, 5) and a["errors_LR"].shape == (4, 5) and a["Q_scale"].shape == (4,)
    # (the uniform quantiser's codes are -k..k with k = 2^(bits - 1) - 1 = 1, dequantised (c / k) * scale)
    for b in range(4):
        s = np.float32(a["Q_scale"][b])
        assert s > 0 and np.unique(a["Q"][b]).tolist() == [-s, 0.0, s]


def test_full_run_keeps_its_fields():
    d = _bench("--full", "--no-cpu-baseline")
    assert all(k in d for k in FULL_ONLY if k != "cpu_baseline")
    assert "cpu_baseline" not in d
    assert d["frob_err_vs_ref_sketch"] < 1e-4
