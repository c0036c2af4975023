"""bench.py as a command on the GPU: a plain run times its steps and nothing
else, --full adds the breakdown, the roofline and the output check, and
--dump-outputs writes the last step's outputs (a small join: every row)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200_003

pytestmark = pytest.mark.gpu


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", "--n", str(N)] + list(args),
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-800:]
    return json.loads(lines[0])


def test_plain_run_and_dump(libs, tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert (d["steps"], d["warmup"], d["unit"], d["dtype"]) == (2, 1, "Mtuples/s", "int64")
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    # value and ms_per_step say the same (ms_per_step is rounded to 1 us)
    assert d["value"] == pytest.approx(2 * N / (d["ms_per_step"] * 1e-3) / 1e6,
                                       rel=0.0006 / d["ms_per_step"] + 1e-3)
    assert d["result_ok"] is True and d["matches"] == N
    # nothing beside the headline figure
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert d["detail"]["kernels_ms_per_step"] == {}
    assert isinstance(d["output_check"], str) and "--full" in d["output_check"]
    got = {f: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["matches.npy", "sorted_R_key.npy", "sorted_R_payload.npy",
                           "sorted_S_key.npy", "sorted_S_payload.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["matches.npy"].tolist() == [float(N)]
    # R: a permutation of the keys 1..N, payload = 5 + its row; S: N foreign keys
    assert np.array_equal(got["sorted_R_key.npy"], np.arange(1, N + 1, dtype=np.float64))
    assert np.array_equal(np.sort(got["sorted_R_payload.npy"]),
                          np.arange(5, N + 5, dtype=np.float64))
    sk = got["sorted_S_key.npy"]
    assert sk.shape == (N,) and (np.diff(sk) >= 0).all() and sk[0] >= 1 and sk[-1] <= N


def test_full_run_keeps_the_rest(libs):
    d = _bench("--full", "--no-cpu-baseline")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["result_ok"] is True and d["matches"] == N
    assert d["output_check"] == {"sorted": True, "checksum_equal": True}
    assert d["roofline"]["kernel"] in d["detail"]["kernels_ms_per_step"]
    assert d["cpu_baseline"] is None
