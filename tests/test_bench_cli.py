"""bench.py command line: --dump-outputs writes the last timed step's
results reproducibly, --full is accepted, and the result line keeps its
contract keys. Runs the tiny model on CPU."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(out_dir, *extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--model", "tiny", "--steps", "3", "--warmup", "1",
         "--batch", "1", "--seq", "128",
         "--dump-outputs", str(out_dir)] + list(extra),
        env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "bench failed:\n%s\n%s" % (p.stdout, p.stderr)
    json_lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1
    rec = json.loads(json_lines[0])
    arrays = {f[:-4]: np.load(os.path.join(str(out_dir), f))
              for f in sorted(os.listdir(str(out_dir)))}
    return rec, arrays


def test_bench_dump_outputs_and_full(tmp_path):
    rec, a = _run_bench(tmp_path / "a")
    rec_full, b = _run_bench(tmp_path / "b", "--full")

    for r in (rec, rec_full):
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step"):
            assert key in r
        assert r["metric"] == "tokens/sec" and r["unit"] == "tokens/s"
        assert r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region
        toks = r["config"]["global_batch"] * r["config"]["seq_len"]
        assert abs(r["value"] * r["ms_per_step"] / 1000.0 - toks) \
            < 1e-6 * toks

    assert set(a) == {"loss", "step_losses", "params", "grads"}
    assert set(b) == set(a)
    total_bytes = 0
    for name, arr in a.items():
        assert arr.dtype == np.float32, name
        assert np.isfinite(arr).all(), name
        total_bytes += arr.nbytes
    assert total_bytes <= 64 << 20
    assert a["loss"].shape == (1,)
    assert a["step_losses"].shape == (3,)      # --steps timed steps
    assert a["loss"][0] == a["step_losses"][-1]
    assert round(float(a["loss"][0]), 4) == rec["config"]["last_loss"]
    assert a["params"].shape == a["grads"].shape and a["params"].size > 0
    assert np.abs(a["grads"]).max() > 0        # a real backward ran

    # same arguments -> same inputs -> the same results run to run
    for name in a:
        assert a[name].shape == b[name].shape, name
        np.testing.assert_allclose(a[name], b[name], rtol=0, atol=1e-6,
                                   err_msg=name)
