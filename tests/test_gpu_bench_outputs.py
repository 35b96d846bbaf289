"""bench.py without --full runs only the headline, and --dump-outputs writes what its last timed step computed: the commitment as
canonical affine limbs, the same point the result line hashes, on the curve, and the same file again for the same arguments
(the inputs come from fixed seeds)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_py as opy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--log-n", "16", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return line, np.load(os.path.join(out_dir, "msm_result_affine.npy"))


def test_dump_outputs_hold_the_last_timed_result(tmp_path):
    line, got = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["extra"] == {}
    assert got.dtype == np.float64 and got.shape == (2, 8) and not line["result_is_infinity"]
    x, y = (sum(int(limb) << (32 * i) for i, limb in enumerate(row)) for row in got)
    assert x < opy.P and y < opy.P and (y * y - x * x * x - 3) % opy.P == 0
    wire = b"".join((v * opy.MONT_R % opy.P).to_bytes(32, "little") for v in (x, y))      # the line hashes the Montgomery form
    assert hashlib.sha256(wire).hexdigest()[:16] == line["result_affine_sha256"]
    _, again = _bench(tmp_path / "b")
    assert np.array_equal(got, again)
