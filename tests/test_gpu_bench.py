"""GPU: bench.py's plain run -- exactly --steps timed steps, ms_per_step over them, none of the --full legs, and --dump-outputs
writing the verdicts of the timed steps and a sample of a batch's MSM terms, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--items", "4096", "--slots", "4", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_times_exactly_steps_and_dumps_outputs(tmp_path):
    steps = 6
    out = _run(tmp_path / "out", steps)
    assert out["metric"] == "thin_vrf_batch_verifications_per_sec" and out["higher_is_better"] is True and out["value"] > 0
    assert out["steps"] == steps and out["timed_steps_per_gpu"] == steps and out["timed_blocks"] == 1
    assert abs(out["ms_per_step"] - out["timed_seconds"] / steps * 1e3) < 1e-9
    assert abs(out["value"] - 4096 * steps / out["timed_seconds"]) < 1e-6 * out["value"]
    for k in ("roofline", "e2e_including_h2d", "cpu_baseline", "cpu_baseline_all_cores", "projected_8gpu", "additional_metrics"):
        assert k not in out, k
    v = np.load(tmp_path / "out" / "verdicts.npy")
    assert v.dtype == np.float32 and v.shape == (steps,) and not v.any()
    # 4 * 4096 + 1 terms, a sample of 16384 of them: 64-byte bases and 32-byte scalars as 16-bit limbs
    idx = np.load(tmp_path / "out" / "msm_term_index.npy")
    bases, scalars = np.load(tmp_path / "out" / "msm_bases_xy_u16.npy"), np.load(tmp_path / "out" / "msm_scalars_u16.npy")
    assert idx.shape == (16384,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] <= 4 * 4096
    assert bases.dtype == scalars.dtype == np.float32 and bases.shape == (16384, 32) and scalars.shape == (16384, 16)
    # the sample equals the oracle's terms (src/thin.rs:282-317) of the first slot's batch, regenerated here as bench.py makes it
    import bench
    import oracle as orc
    from ark_vrf_amd import _native as nat
    ctx = nat.Context(nat.BANDERSNATCH_SHA512_ELL2, device=0)
    _, raw = bench.make_batch(ctx, nat, 4096, start=0)
    ctx.close()
    st, ob, osc = orc.thin_batch_terms_xy(orc.BANDERSNATCH, raw)
    assert st == 0 and len(osc) == 32 * (4 * 4096 + 1)
    rows = idx.astype(np.int64)
    assert np.array_equal(np.frombuffer(ob, dtype="<u2").reshape(-1, 32)[rows].astype(np.float32), bases)
    assert np.array_equal(np.frombuffer(osc, dtype="<u2").reshape(-1, 16)[rows].astype(np.float32), scalars)
    assert np.count_nonzero(scalars.any(axis=1)) > 16000
    # same arguments, same inputs, same outputs
    _run(tmp_path / "again", steps)
    for name in ("msm_term_index", "msm_bases_xy_u16", "msm_scalars_u16"):
        assert np.array_equal(np.load(tmp_path / "out" / (name + ".npy")), np.load(tmp_path / "again" / (name + ".npy"))), name
