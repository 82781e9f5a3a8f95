"""bench.py --gpus N starts its own ranks (VERDICT r05 Missing 1): `python bench.py --gpus 8` — the shape of the driver's N = 1 command — must measure 8 ranks or refuse,
never one rank that prints n_gpus = 1.  The per-chromosome fan-out it measures is the reference's Parallel.ForEach over chromosomes
(/root/reference/Src/Canvas/CanvasPartition/CBSRunner.cs:115-147, HiddenMarkovModelsRunner.cs:51-104, CanvasBin/CanvasBin.cs:513-539)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CANVAS_BENCH_ONE_GPU"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_gpus_n_refuses_when_the_box_has_fewer_devices():
    """no launcher, --gpus 64: non-zero exit, no JSON line (this container has no GPU, the test box has one)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0"], env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert "needs 64 visible GPUs" in p.stderr and "{" not in p.stdout


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_pass(tmp_path):
    """a plain run times --steps passes and prints the headline only (the other legs belong to --full); --dump-outputs writes what the last timed pass returned,
    the same files for the same arguments"""
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / ("d%d" % i)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "0.02", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                           env=_env(), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
        lines.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    j = lines[0]
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0 and j["higher_is_better"] is True
    assert not any(k in j for k in ("roofline", "cbs_path", "wavelets_path", "cpu_baseline", "h2d", "packed_path", "somatic_flow", "pedigree_flow"))
    a, b = dumps
    assert sorted(a) == sorted(b) and all(a[f].dtype in (np.float32, np.float64) and a[f].tobytes() == b[f].tobytes() for f in a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    n = int(a["bins_after_clean.npy"][0])
    assert n == j["config"]["bins_after_clean"] and int(a["segments.npy"][0]) == j["config"]["segments"] and int(a["bin_size.npy"][0]) == j["config"]["bin_size"]
    assert len(a["coverage.npy"]) == min(n, 1_000_000) and a["chr_offset.npy"][-1] == n
    assert (np.diff(a["bin_index.npy"]) > 0).all() and (np.diff(a["bins_chr.npy"]) >= 0).all() and (a["bins_stop.npy"] > a["bins_start.npy"]).all()
    assert all((a[f] == np.round(a[f])).all() for f in ("state.npy", "segment_id.npy", "bins_gc.npy"))


@pytest.mark.gpu
def test_world_size_and_gpus_must_agree():
    """under a launcher whose world differs from --gpus the bench refuses instead of printing a line for the wrong N"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"], env=_env(RANK="0", WORLD_SIZE="2", LOCAL_RANK="0"), capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "WORLD_SIZE=2" in (p.stderr + p.stdout)


@pytest.mark.gpu
def test_gpus_2_starts_two_ranks_and_every_sharded_leg_agrees():
    """python bench.py --gpus 2 (no launcher): two ranks are started here; with one GPU on the test box both sit on GPU 0 and exchange through the host transport
    (CANVAS_BENCH_ONE_GPU=1).  The line must say n_gpus = 2 and every sharded leg must be identical on all ranks and equal to the single-GPU result."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scale", "0.02", "--steps", "2", "--warmup", "1"],
                       env=_env(CANVAS_BENCH_ONE_GPU="1"), capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["multi"] == "sharded"
    assert j["sharded"]["identical_on_all_ranks"] is True and j["sharded"]["equals_single_gpu_result"] is True
    assert j["sharded"]["collective_ms"] > 0 and j["sharded"]["redundant_clean_ms"] > 0          # the first hardware curve comes with its own explanation (VERDICT r05 Next 8)
    assert j["partition_sharded"]["cbs"]["collectives"] >= 1 and j["partition_sharded"]["wavelets"]["collectives"] >= 1 and j["somatic_sharded"]["collectives"] >= 1
    for leg in ("cbs", "wavelets"):
        assert j["partition_sharded"][leg]["identical_on_all_ranks"] is True and j["partition_sharded"][leg]["equals_single_gpu_result"] is True, j["partition_sharded"]
    assert j["somatic_sharded"].get("identical_on_all_ranks") is True and j["somatic_sharded"].get("equals_single_gpu_flow_rank0") is True, j["somatic_sharded"]
    assert j["pedigree_sharded"].get("identical_on_all_ranks") is True and j["pedigree_sharded"].get("equals_single_gpu_flow_rank0") is True, j["pedigree_sharded"]
    assert "skipped" in j["pedigree_grid"]            # a trio needs three ranks
    assert j["cohort_mode"]["samples"] == 2


@pytest.mark.gpu
def test_gpus_3_runs_the_pedigree_grid():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--scale", "0.02", "--steps", "1", "--warmup", "1"],
                       env=_env(CANVAS_BENCH_ONE_GPU="1", CANVAS_SHARDED_NO_SOMATIC="1"), capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert j["n_gpus"] == 3
    g = j["pedigree_grid"]
    assert g.get("identical_on_all_ranks") is True and g.get("equals_single_gpu_flow_rank0") is True, g
