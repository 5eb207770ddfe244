"""`python bench.py --gpus N` must really run N ranks (round-1 verdict: `--gpus` was parsed and ignored).  The launcher part is
exercised on CPU with --dry-run (rendezvous, barrier, all-reduce over gloo, the one JSON line, exit codes); the full path with two
ranks sharing the one GPU of the test box over gloo is the -m gpu case."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([sys.executable, BENCH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_gpus_flag_starts_that_many_ranks():
    rc, out, err = run(["--gpus", "2", "--dry-run", "--steps", "3"])
    assert rc == 0, err
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, f"exactly one line on stdout, got {lines!r}"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] is None


@pytest.mark.parametrize("gpus,total,name", [(4, 64, "configs[3]"), (8, 128, "configs[4]")])
def test_default_multi_gpu_workload_is_the_baseline_config(gpus, total, name):
    """`bench.py --gpus N` without --particles: 16 M particles per GPU, i.e. BASELINE configs[3] on 4 GPUs (64 M, 2x2) and configs[4]
    on 8 (128 M, strips) — what a driver run with only --steps/--warmup times."""
    rc, out, err = run(["--gpus", str(gpus), "--dry-run"])
    assert rc == 0, err
    d = json.loads([ln for ln in out.splitlines() if ln.strip()][-1])
    wl = d["config"]["workload"]
    assert d["n_gpus"] == gpus and d["config"]["particles_per_gpu"] == 16_000_000
    assert name in wl and f"{total} M" in wl, wl
    n_total = int(wl.split("~")[1].split(" ")[0])
    assert abs(n_total - total * 1_000_000) < 0.01 * total * 1_000_000, wl


def test_single_gpu_default_workload_is_the_largest_single_gpu_config():
    """`python bench.py` / `--gpus 1`: the headline is BASELINE configs[2], 16 M particles — the size where the HBM roofline binds
    (VERDICT r03 item 3); the 1 M windows ride in `also`."""
    rc, out, err = run(["--dry-run"])
    assert rc == 0, err
    d = json.loads([ln for ln in out.splitlines() if ln.strip()][-1])
    assert d["n_gpus"] == 1 and d["config"]["particles_per_gpu"] == 16_000_000
    n_total = int(d["config"]["workload"].split("~")[1].split(" ")[0])
    assert abs(n_total - 16_000_000) < 160_000


def test_ranks_started_by_an_external_launcher_get_the_dmabuf_ipc_variable():
    """The driver starts the N > 1 bench as `python -m torch.distributed.run ... bench.py --gpus N`: bench.py's own launcher (which sets
    HSA_ENABLE_IPC_MODE_LEGACY=0 for its children) is not involved, so every rank must set it itself before anything loads the HIP
    runtime."""
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
                        str(port), BENCH, "--gpus", "2", "--dry-run"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["config"]["launcher"].startswith("external")
    assert d["config"]["HSA_ENABLE_IPC_MODE_LEGACY_per_rank"] == ["0", "0"]


def test_dry_run_can_time_the_scene_build_of_every_rank():
    """`--dry-run --dry-run-scene`: every rank builds the GLOBAL scene like a real N-rank run does before it cuts its tile; the line carries
    the slowest rank's seconds (what DESIGN.md section 7 quotes for 8 ranks x 128 M particles)."""
    rc, out, err = run(["--gpus", "2", "--dry-run", "--dry-run-scene", "--particles", "20000"])
    assert rc == 0, err
    c = json.loads([ln for ln in out.splitlines() if ln.strip()][-1])["config"]
    assert 39_000 < c["scene_particles"] < 41_000 and c["scene_build_seconds_max_over_ranks"] > 0.0


def test_world_size_must_match_gpus():
    rc, out, err = run(["--gpus", "2", "--dry-run"], env={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert rc != 0 and out.strip() == ""
    assert "torch.distributed.run" in err and "--gpus 2" in err  # the message names the exact command


def test_more_ranks_than_gpus_fails_loudly():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 GPUs")
    rc, out, err = run(["--gpus", "2", "--steps", "1"])
    assert rc != 0 and out.strip() == "" and "GPU(s) are visible" in err


@pytest.mark.gpu
def test_two_ranks_share_the_gpu_over_gloo():
    """The whole multi-rank path without a launcher: 2 ranks (tiles) on the one GPU of the box, halo records staged through gloo."""
    rc, out, err = run(["--gpus", "2", "--backend", "gloo", "--particles", "20000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    assert rc == 0, err[-2000:]
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_seen"] == 2 and d["value"] > 0
    assert d["config"]["particles_total"] > 30000
    # measured, not assumed: list statistics and ownership come from the tiles
    assert 6.0 < d["config"]["mean_neighbors"] < 14.0 and d["step_model"]["k_and_r"].startswith("measured")
    assert len(d["config"]["owned_particles_per_rank"]) == 2 and sum(d["config"]["owned_particles_per_rank"]) == d["config"]["particles_total"]
    assert "transport" in d["config"]


@pytest.mark.gpu
def test_four_ranks_on_2x2_tiles_share_the_gpu_over_gloo():
    """configs[3]'s layout through the launcher-free multi-rank path: 4 ranks = 2 x 2 tiles (three neighbours each, diagonal ones
    included) on the one GPU of the box, halo records staged through gloo; most exchanges packed from the density correction's
    classification."""
    rc, out, err = run(["--gpus", "4", "--backend", "gloo", "--particles", "60000", "--steps", "12", "--warmup", "2", "--no-cpu-baseline", "--no-roofline"])
    assert rc == 0, err[-2000:]
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["world_size_seen"] == 4 and d["value"] > 0
    c = d["config"]
    assert "2 x N/2" in c["parallelism"] and "3 neighbours" in c["parallelism"], c["parallelism"]
    assert len(c["owned_particles_per_rank"]) == 4 and sum(c["owned_particles_per_rank"]) == c["particles_total"]
    assert 6.0 < c["mean_neighbors"] < 14.0
    packed = int(c["parallelism"].split(" exchanges (")[1].split(" ")[0])
    total = int(c["parallelism"].split(" exchanges (")[0].split(" ")[-1])
    assert total >= 14 and packed >= total - 4, c["parallelism"]


def test_bench_refuses_zero_steps_and_multi_rank_dumps():
    rc, out, err = run(["--steps", "0", "--dry-run"])
    assert rc != 0 and out.strip() == "" and "--steps" in err
    rc, out, err = run(["--gpus", "2", "--dry-run", "--dump-outputs", "unused"])
    assert rc != 0 and out.strip() == "" and "--dump-outputs" in err


def test_full_flag_is_accepted():
    rc, out, err = run(["--dry-run", "--full", "--steps", "4"])
    assert rc == 0, err
    d = json.loads([ln for ln in out.splitlines() if ln.strip()][-1])
    assert d["steps"] == 4


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_every_time(tmp_path):
    """A plain run times exactly --steps steps and carries none of --full's extras; --dump-outputs writes the last timed step's arrays,
    identical from run to run with the same arguments."""
    lines = []
    for k in range(2):
        rc, out, err = run(["--particles", "20000", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / f"run{k}")])
        assert rc == 0, err[-2000:]
        ls = [ln for ln in out.splitlines() if ln.strip()]
        assert len(ls) == 1
        lines.append(json.loads(ls[0]))
    for d in lines:
        assert d["steps"] == 7 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] - d["config"]["particles_total"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert "roofline" not in d and "also" not in d and "cpu_baseline" not in d
    import numpy as np

    names = sorted(os.listdir(tmp_path / "run0"))
    assert names == ["densities.npy", "last_step_stats.npy", "positions.npy", "sample_index.npy", "timer.npy", "velocities.npy"]
    assert sorted(os.listdir(tmp_path / "run1")) == names
    n = lines[0]["config"]["particles_total"]
    for name in names:
        a, b = np.load(tmp_path / "run0" / name), np.load(tmp_path / "run1" / name)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        assert np.array_equal(a, b), name
    assert np.load(tmp_path / "run0" / "positions.npy").shape == (n, 2)  # fewer than 2^20 particles: all of them, in array order
    assert np.array_equal(np.load(tmp_path / "run0" / "sample_index.npy"), np.arange(n))
    assert np.load(tmp_path / "run0" / "last_step_stats.npy").shape == (12,)


@pytest.mark.gpu
def test_full_run_adds_the_roofline_record():
    rc, out, err = run(["--full", "--particles", "20000", "--steps", "8", "--warmup", "2", "--no-cpu-baseline"])
    assert rc == 0, err[-2000:]
    ls = [ln for ln in out.splitlines() if ln.strip()]
    assert len(ls) == 1
    d = json.loads(ls[0])
    assert d["steps"] == 8 and d["value"] > 0 and d["roofline"]["kernel"] and d["roofline"]["per_kernel"]
