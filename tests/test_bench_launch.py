"""bench.py as the driver calls it: `python bench.py --gpus N --steps K --warmup W`, with and without a launcher
(replaces the reference's single-process loop, cald_train.py:434-447, and the pickled all_gather of
detection/utils.py:75-115).  The GPU tests run the N = 2 command on whatever the box has: RCCL across two devices when two are
visible, two ranks sharing the one GPU over gloo otherwise -- the JSON line says which."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = ["--no-cpu-baseline", "--no-full-pool", "--no-f16x3", "--no-train", "--no-cfg4"]


def _run(argv, env=None, timeout=900):
    e = dict(os.environ, **(env or {}))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable] + argv, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None), lines


def test_self_launch_fails_loudly_without_a_gpu():
    """No GPU -> every rank refuses (no CPU fallback), the launcher reaps its ranks and returns non-zero instead of hanging
    or printing a number."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-box behaviour")
    p, line, _ = _run(["bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"] + FAST, timeout=300)
    assert p.returncode != 0
    assert line is None
    assert "needs an MI355X" in p.stderr


@pytest.mark.gpu
def test_bench_two_ranks_self_launched_equals_one_rank():
    """The driver's command, unchanged, for N = 1 and N = 2: rc 0, ONE JSON line, n_gpus == N, both ranks seen through the
    collective, the same fixed pool (strong scaling) -> the SAME selected indices as the 1-rank run."""
    args = ["--steps", "2", "--warmup", "1"] + FAST
    p1, one, l1 = _run(["bench.py", "--gpus", "1"] + args)
    assert p1.returncode == 0, p1.stderr[-2000:]
    p2, two, l2 = _run(["bench.py", "--gpus", "2"] + args)
    assert p2.returncode == 0, p2.stderr[-2000:]
    assert len(l1) == 1 and len(l2) == 1
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert one["scaling"] == two["scaling"] == "strong"
    assert one["config"]["pool_images"] == two["config"]["pool_images"] == 128
    assert two["config"]["selected_sha1"] == one["config"]["selected_sha1"]
    assert two["config"]["n_selected"] == one["config"]["n_selected"] > 0
    r = two["rccl"]
    assert r["world_size"] == 2 and r["ranks_seen"] == 2
    assert sorted(x["rank"] for x in r["per_rank"]) == [0, 1]
    assert sum(x["images"] for x in r["per_rank"]) == 128
    import torch
    if torch.cuda.device_count() >= 2:
        assert r["backend"] == "nccl" and r["distinct_devices"] == 2 and not r["shared_gpu"]
        # with a GPU per rank the score rows travel through the C ABI's own collective (cald_allgather_scores), not torch.distributed
        assert r["cabi"]["world_size"] == 2 and "cald_allgather_scores" in r["collective"]
    else:
        assert r["backend"] == "gloo" and r["shared_gpu"] and r["cabi"] is None
    assert abs(two["ms_per_step"] * two["steps"] - 128 / two["value"] * 1e3) < 1e-3 * two["ms_per_step"] * two["steps"] + 1e-6


@pytest.mark.gpu
def test_bench_under_torch_distributed_run_weak_scaling():
    """The launcher form of the contract (`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`) and the
    weak-scaling option: K x 64 images per rank."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    p, line, lines = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "1",
                           "--scaling", "weak"] + FAST)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["pool_images"] == 128
    assert line["rccl"]["ranks_seen"] == 2 and [x["images"] for x in line["rccl"]["per_rank"]] == [64, 64]


@pytest.mark.gpu
def test_bench_cabi_collective_falls_back_together_when_a_rank_cannot_join():
    """`--comm cabi` on a box where RCCL cannot form the communicator (two ranks on ONE device: ncclCommInitRank returns 'invalid usage'):
    every step of the bootstrap is agreed on through the launcher's process group, so all ranks leave the C-ABI path TOGETHER, the rows
    travel through torch.distributed, rc is 0, there is ONE JSON line, it says what happened -- nobody is left alone in a collective."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box where RCCL refuses the communicator (one visible GPU)")
    p, line, lines = _run(["bench.py", "--gpus", "2", "--comm", "cabi", "--steps", "2", "--warmup", "1"] + FAST, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1 and line["n_gpus"] == 2
    r = line["rccl"]
    assert r["ranks_seen"] == 2 and r["backend"] == "gloo"
    assert "error" in r["cabi"] and "cald_comm_init_rank" in r["cabi"]["error"]
    assert line["config"]["n_selected"] > 0


def test_dump_outputs_writes_what_the_timed_path_returned(tmp_path, monkeypatch):
    """--dump-outputs: consistency / cls_corr / selected indices as float64 .npy; above the cap a fixed seeded sample of the per-image
    rows (same rows run to run, their numbers in sample_rows.npy) and the whole selection, all within the cap."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rs = np.random.RandomState(3)
    cons, cls, picked = rs.rand(640), rs.rand(640, 20), rs.permutation(640)[:61]
    bench.dump_outputs(str(tmp_path / "a"), cons, cls, picked)
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("consistency", "cls_corr", "selected_indices")}
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["cls_corr.npy", "consistency.npy", "selected_indices.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["consistency"], cons) and np.array_equal(got["cls_corr"], cls)
    assert np.array_equal(got["selected_indices"], picked.astype(np.float64))
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1 << 20)
    n = 20000                                                       # 20 000 x 21 doubles = 3.4 MB > the 1 MB cap
    cons, cls = rs.rand(n), rs.rand(n, 20)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), cons, cls, picked)
    size = sum(os.path.getsize(str(tmp_path / "b" / f)) for f in os.listdir(str(tmp_path / "b")))
    assert size <= 1 << 20
    rows = np.load(str(tmp_path / "b" / "sample_rows.npy")).astype(np.int64)
    assert np.array_equal(rows, np.load(str(tmp_path / "c" / "sample_rows.npy")))
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(str(tmp_path / "b" / "consistency.npy")), cons[rows])
    assert np.array_equal(np.load(str(tmp_path / "b" / "cls_corr.npy")), cls[rows])
    assert np.array_equal(np.load(str(tmp_path / "b" / "selected_indices.npy")), picked.astype(np.float64))


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run carries the headline only (no leg that takes a run of its own), `ms_per_step` x `steps` is the timed region, and
    --dump-outputs writes the timed pool's scores and selection: the same inputs give the same arrays in a second run."""
    import numpy as np
    outs = []
    for d in ("a", "b"):
        p, line, lines = _run(["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / d)])
        assert p.returncode == 0, p.stderr[-2000:]
        assert len(lines) == 1 and line["steps"] == 1
        for leg in ("full_pool", "cpu_baseline", "config0_cpu_plumbing", "f16x3_mode", "cfg4_f16x3", "training_step", "parity_vs_independent_fp32"):
            assert leg not in line, leg
        assert abs(line["ms_per_step"] - 64 / line["value"] * 1e3) < 1e-3 * line["ms_per_step"]
        outs.append({n: np.load(str(tmp_path / d / (n + ".npy"))) for n in ("consistency", "cls_corr", "selected_indices")})
        assert outs[-1]["consistency"].shape == (64,) and outs[-1]["cls_corr"].shape == (64, 20)
        assert len(outs[-1]["selected_indices"]) == line["config"]["n_selected"]
    assert all(np.array_equal(outs[0][n], outs[1][n]) for n in outs[0])
