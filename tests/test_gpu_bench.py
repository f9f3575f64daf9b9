"""The benchmark's multi-rank path on the GPU box: a plain
`python bench.py --gpus 2` starts its own two ranks (torch.distributed.run on
127.0.0.1), each renders its interleaved-row shard of config 3, the shards
are gathered and de-interleaved on rank 0, and the gathered frame is checked
bit for bit against rank 0 rendering the whole frame alone.  With one GPU on
the box both ranks share it over gloo (BWRT_DIST_BACKEND=gloo); on an 8-GPU
node the same path runs one rank per GPU over RCCL."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_plain_launch_two_ranks_verified():
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BWRT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints the one JSON line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_size"] == 2 and out["backend"] == "gloo"
    assert out["verified"] is True, out.get("verify")
    assert out["value"] > 0 and out["config"]["parallelism"].startswith("pixel-rows/2")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_plain_run_dumps_last_step(tmp_path, bwrt_lib):
    """A plain `bench.py --gpus 1 --steps 2 --warmup 1` times exactly its
    steps and carries no CPU-baseline leg; --dump-outputs writes the last
    step's frame and frameSum, which a renderer taking the same three
    renders from the same seeds reproduces bit for bit."""
    import numpy as np
    from bwrt import Renderer, scenes
    env = {k: v for k, v in os.environ.items() if k == "BWRT_LIB" or not k.startswith("BWRT_")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0 and out["unit"] == "Msamples/s" and out["dtype"] == "f32"
    assert abs(out["value"] - 1920 * 1080 * 8 * 4 / out["ms_per_step"] / 1e3) <= 1e-3 * out["value"]
    assert "cpu_baseline" not in out and "oracle_check" not in out and out["verified"] is None
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("image", "frame_sum", "rows")}
    assert got["image"].dtype == np.float32 and got["image"].shape == (1080, 1920, 4)
    assert got["frame_sum"].dtype == np.float32 and got["frame_sum"].shape == (1080, 1920, 3)
    assert np.array_equal(got["rows"], np.arange(1080))
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_scene(scenes.SCENES["07"]())
        g.init_rand(1920, 1080)
        for _ in range(3):  # 1 warm-up + 2 timed steps, the RNG streams continuing
            img, acc = g.render(1920, 1080, 8, 4, first_frame=1, want_accum=True)
    assert np.array_equal(got["image"], img.astype(np.float32))
    assert np.array_equal(got["frame_sum"], acc, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_rccl_path_one_rank_verified():
    """The RCCL branch every N > 1 point of the headline takes (nccl process
    group with device_id, rooted gather of the row blocks on the gather
    stream, de-interleave kernel, verify against a solo render), run once at
    world size 1 under torch.distributed.run with the default backend."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                        "BWRT_DIST_BACKEND")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
                        "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "bench.py"),
                        "--gpus", "1", "--dist", "--steps", "3", "--warmup", "1"],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["backend"] == "rccl" and out["world_size"] == 1 and out["n_gpus"] == 1
    assert out["verified"] is True, out.get("verify")
    assert "rccl gather" in out["config"]["parallelism"]
