"""bench.py for N > 1 on the one GPU of the test box, both ways it gets started: as the driver launches it
(torch.distributed.run, one process per rank) and as a plain `python bench.py --gpus 2` (bench.py starts its own
ranks).  Both ranks share cuda:0 and talk over gloo (AMMC_BENCH_SHARE_GPU=1).  Checks the single JSON line, the
whole-job aggregation and all three modes."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


UNITS = {"infer": 4, "train": 2, "stress": 2 * 1024}


@pytest.mark.parametrize("launcher", ["torchrun", "self"])
@pytest.mark.parametrize("mode,extra", [("infer", ["--batch", "4", "--size", "64", "--no-cpu-baseline", "--full"]),
                                         ("train", ["--batch", "2", "--size", "64"]),
                                         ("stress", ["--batch", "2"])])
def test_bench_two_ranks(mode, extra, launcher):
    env = dict(os.environ, AMMC_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--mode", mode] + extra
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port())] + tail
    else:
        cmd = [sys.executable] + tail                                # bench.py spawns the two ranks itself
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]                      # rank 0 prints ONE line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["scaling"] == "weak" and rec["higher_is_better"] is True
    assert rec["rccl_ranks"] == 2                                   # read back from dist.get_world_size()
    per_step = 2 * UNITS[mode]                                      # whole-job units per step = sum over ranks
    assert abs(rec["value"] - per_step / (rec["ms_per_step"] * 1e-3)) <= 0.02 * rec["value"]
    if mode == "infer":
        assert rec["roofline"]["bound"] == "mfma" and rec["roofline"]["frac"] > 0
    if mode == "train":
        # what the one-shot 8-GPU run needs to be interpretable (round-4 review, item 8): the channel cap in force, how many
        # gradient buckets a step launches and what the collectives cost the step's stream beyond what the backward hid
        col = rec["collectives"]
        assert "nccl_max_nchannels" in rec and "nccl_max_nchannels" in col
        assert col["gradient_buckets_per_step"] >= 1 and col["bucket_mb"] == 25.0
        assert col["exposed_ms_per_step"]["median"] >= 0.0 and col["exposed_ms_per_step"]["max"] >= col["exposed_ms_per_step"]["median"]


@pytest.mark.parametrize("mode,extra,units", [("infer", ["--batch", "1", "--size", "64", "--no-cpu-baseline"], 1),
                                               ("train", ["--batch", "1", "--size", "64"], 1),
                                               ("train", ["--batch", "1", "--size", "64", "--sync-stats"], 1),
                                               ("stress", ["--batch", "1"], 1024)])
def test_bench_eight_ranks_self_spawned(mode, extra, units):
    """the shape of the driver's 8-GPU run on the one test GPU: `python bench.py --gpus 8` starts eight ranks itself
    (port handling, RANK / LOCAL_RANK / WORLD_SIZE, teardown), every rank runs its share, rank 0 prints ONE line whose
    value is the sum over the eight ranks and whose `rccl_ranks` is read back from the process group"""
    env = dict(os.environ, AMMC_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--mode", mode] + extra
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["rccl_ranks"] == 8 and rec["scaling"] == "weak"
    assert abs(rec["value"] - 8 * units / (rec["ms_per_step"] * 1e-3)) <= 0.02 * rec["value"]
    if mode == "train":                                              # the lock-step statistics collectives of 8 ranks
        assert rec["config"]["statistics_collectives_per_step"] == (33 if "--sync-stats" in extra else 0)


def test_bench_refuses_more_ranks_than_gpus():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "AMMC_BENCH_SHARE_GPU")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "GPU(s) visible" in out.stderr
