"""bench.py's command line on the smallest workload (c1: 500 nodes): a plain run prints the headline line alone, times
exactly --steps steps and, with --dump-outputs, writes the last timed step's results, which are the oracle's; --full adds
the roofline, the single-pod calls, the PCIe-inclusive step, the oracle check and the CPU baseline to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, PER_STEP = 3, 3300  # the third step still places pods and already meets unschedulable ones
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "placed")
FULL_ONLY = ("roofline", "cpu_baseline", "pcie_inclusive_pods_per_sec", "single_pod_call", "oracle_check")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c1", "--steps",
                        str(STEPS), "--warmup", "1", "--pods-per-step", str(PER_STEP), *extra],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    out, err = _bench("--profile-pods", "0", "--single-pod-calls", "0", "--dump-outputs", str(tmp_path / "dump"))
    for k in HEADLINE:
        assert k in out, k
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["steps"] == STEPS and err.count("[bench] step ") == STEPS
    assert out["unit"] == "pods/s" and out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(PER_STEP / (out["ms_per_step"] * 1e-3), rel=1e-9)

    import bench
    from koordinator_amd import framework
    from oracle import oracle
    cfg = framework.build_config(batch_pods=32, pods_per_wave=8, device_id=0)
    work = bench.Work("c1", 500, cfg)
    pods = work.make_pods(STEPS * PER_STEP, seed=work.seed + 1)
    want_node, want_score, _ = oracle.schedule_cluster(cfg, work.cluster, pods)
    assert out["placed"] == int((want_node >= 0).sum())
    last = slice((STEPS - 1) * PER_STEP, STEPS * PER_STEP)
    assert 0 < (want_node[last] >= 0).sum() < PER_STEP
    node, score = np.load(tmp_path / "dump" / "node.npy"), np.load(tmp_path / "dump" / "score.npy")
    assert sorted(os.listdir(tmp_path / "dump")) == ["node.npy", "score.npy"]
    assert node.dtype == np.float64 and score.dtype == np.float64
    np.testing.assert_array_equal(node, want_node[last].astype(np.float64))
    np.testing.assert_array_equal(score, want_score[last].astype(np.float64))


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    out, _ = _bench("--full", "--cpu-seconds", "0.3", "--single-pod-calls", "20", "--profile-pods", "500")
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["steps"] == STEPS and out["oracle_check"] is True
    import bench
    assert out["oracle_check_live_pods"] == min(bench.WORKLOADS["c1"][4], STEPS * PER_STEP)
    assert out["cpu_baseline"]["value"] > 0 and out["single_pod_call"]["calls"] == 20
    assert out["roofline"]["kernel"] == "eval_round" and out["roofline"]["kernel_ms"] > 0


def test_steps_default_and_explicit_value():
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py"]
        assert bench.parse().steps is None and bench.parse().full is False and bench.parse().dump_outputs is None
        sys.argv = ["bench.py", "--workload", "c1", "--steps", "10", "--full", "--dump-outputs", "d"]
        a = bench.parse()
        assert (a.steps, a.full, a.dump_outputs) == (10, True, "d")
    finally:
        sys.argv = argv
