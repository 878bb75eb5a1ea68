#!/usr/bin/env python
"""bench.py -- CALD consistency sweep throughput on MI355X (unlabeled images scored / second).

Workload = BASELINE.json configs[1]: Faster R-CNN ResNet-50 FPN, 21 classes, min/max size 600/1000, augmentations flip /
cut_out / smaller_resize, seeded pseudo-trained weights (cald_amd/synth.py), float32 (exact fp32 MFMA), on a pool of
synthetic VOC2012-shaped baseline-JPEG files.

A "step" is one pass of the hot path (cald_sweep: reference view + 3 augmented views per image, detector forward x4,
consistency scoring) over one batch of 64 pool images.  The timed region (SURVEY.md section 8d metric) is
    K steps over a pool of K x 64 images per GPU that is resident in HBM (decoded once on the GPU from the JPEG bytes,
    cald_amd/pool.py)  ->  one all-gather of the per-image score rows (N > 1)  ->  argsort + cls_kldiv selection on the
    host  ->  selected indices available,
bracketed by barrier + synchronize; `value` = images of all ranks / max-over-ranks time.  The JPEG decode + H2D of the
same pool is timed right before it and reported as `from_host_jpeg_bytes` (PCIe- and decode-inclusive rate; never
`value`).  With --full, at N = 1 the headline run additionally sweeps the FULL configs[1] pool (5 217 images: host JPEG bytes ->
selected 500 indices, everything inside one clock) and reports it as `full_pool`.

    python bench.py --gpus N --steps K --warmup W [--scaling strong|weak]
N > 1: one rank per GPU.  Either launch it with torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the
environment) or call it plainly -- `python bench.py --gpus N ...` then starts its own N ranks (launch_ranks).  Backend =
RCCL ("nccl") when N GPUs are visible, otherwise the ranks share the visible GPU(s) over gloo (RCCL refuses two ranks
on one device), which the JSON line says (`rccl`).  The pool is sharded by position (rank-local inputs, no data-path
collective) and one all-gather of the score rows closes the timed region.  Prints ONE JSON line on rank 0.

--scaling strong (default, SURVEY 8d: a FIXED pool / wall time): K x 64 images in total, split over the N ranks; without
--steps the pool is the whole configs[1] pool of 5 217 images.  --scaling weak: K x 64 images per GPU.

A plain run does only what the headline needs: set up, warm up, time the K steps, print the line (`ms_per_step` = the timed
region / K).  --full adds everything else the line used to carry, each in runs of its own after the timed region: `full_pool`,
`cpu_baseline` + `config0_cpu_plumbing`, `f16x3_mode`, `cfg4_f16x3`, `training_step` (each still switched off by its --no-* option)
and `parity_vs_independent_fp32`.  --dump-outputs DIR writes what the timed path returned (consistency [n] f64, cls_corr [n, C-1]
f64, the selected pool indices as f64) to DIR/*.npy; the pool and the weights are seeded, so the same arguments give the same inputs.
"""
import argparse
import hashlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs @ 2.4 GHz
F16_MFMA_PEAK_TFLOPS = 2516.6  # v_mfma_f32_32x32x16_f16: 32 cycles / SIMD -> 16 x the f32-input rate (dense)
FULL_POOL = 5217               # VOC2012 train 5 717 - 500 initially labeled (cald_train.py:299-300)
FULL_BUDGET = 500


def usable_cpus():
    """CPUs this process may really use: the scheduler affinity capped by the cgroup quota (the GPU boxes grant 16 of the
    host's cores through cpu.max, which os.cpu_count() does not show)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (same environment contract as
    torch.distributed.run: RANK, LOCAL_RANK, WORLD_SIZE, LOCAL_WORLD_SIZE, MASTER_ADDR, MASTER_PORT), rank 0 inherits
    stdout (the one JSON line), and the first failing rank takes the job down (children are killed by PID)."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", CALD_BENCH_SELF_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc, live = 0, list(procs)
    while live:
        time.sleep(0.2)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in live:
                    q.terminate()
    return rc


def exchange_id_over_tcp(rank, world, uid, timeout_s=120.0):
    """Ships the 128-byte RCCL unique id from rank 0 to every rank over a plain TCP socket on MASTER_ADDR : MASTER_PORT + 29 (the
    launcher's rendezvous port stays torch's).  Stands for "any means" of include/cald_hip.h -- a C host would do the same."""
    import socket
    host = os.environ.get("MASTER_ADDR", "127.0.0.1")
    port = int(os.environ.get("MASTER_PORT", "29500")) + 29
    if rank == 0:
        srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        srv.bind((host, port)); srv.listen(world); srv.settimeout(timeout_s)
        try:
            for _ in range(world - 1):
                c, _addr = srv.accept()
                c.sendall(uid); c.close()
        finally:
            srv.close()
        return uid
    t0 = time.time()
    while True:
        try:
            c = socket.create_connection((host, port), timeout=5.0)
            break
        except OSError:
            if time.time() - t0 > timeout_s:
                raise
            time.sleep(0.05)
    buf = b""
    while len(buf) < 128:
        chunk = c.recv(128 - len(buf))
        if not chunk:
            raise RuntimeError("rank 0 closed the id socket early")
        buf += chunk
    c.close()
    return buf


def _jpeg_of(args):
    """(pool position, (H, W)) -> baseline JPEG bytes of the synthetic image (runs in forked host workers)."""
    pos, (H, W) = args
    from PIL import Image
    from cald_amd import synth
    b = io.BytesIO()
    Image.fromarray(synth.synth_image(pos, H, W)).save(b, format="JPEG", quality=90)
    return b.getvalue()


def make_jpeg_pool(positions, sizes):
    """Synthetic pool as JPEG byte strings, generated on the host cores BEFORE anything touches the GPU (fork is only
    safe then).  Not timed: stands for the files of the dataset directory."""
    import multiprocessing as mp
    jobs = [(p, sizes[p]) for p in positions]
    nproc = max(1, min(64, usable_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))))
    if nproc == 1 or len(jobs) < 8:
        return [_jpeg_of(j) for j in jobs]
    with mp.get_context("fork").Pool(nproc) as pool:
        return pool.map(_jpeg_of, jobs, chunksize=8)


def synthetic_labeled_set(n=500, num_cls=21, seed=0):
    """Class labels of the initially labeled images (what cls_kldiv reads from labeled_loader, cald_train.py:237-242)."""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed)
    return [(None, [{"labels": torch.from_numpy(rs.randint(1, num_cls, rs.randint(1, 6)))}]) for _ in range(n)]


def cpu_baseline(sd, blobs, augs, positions, gpu_scores, budget_s=48.0, max_images=32):
    """The reference-shaped PyTorch-CPU port (oracle/torch_port.py) on a bounded sample of the same workload."""
    import numpy as np
    import torch
    from PIL import Image
    from oracle import torch_port
    pool = [np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in blobs[:max_images]]
    model = torch_port.TorchFRCNN(sd, 21, 50, 600, 1000)
    model.forward(pool[0])          # warm-up view (oneDNN primitive creation), not timed
    # batch-1 convolutions do not scale to every core of a big host: use the thread count that is fastest here
    default_threads = torch.get_num_threads()
    best = (None, 1e30)
    for nt in sorted({default_threads, max(1, default_threads // 2), max(1, default_threads // 4), max(1, default_threads // 8)}, reverse=True):
        torch.set_num_threads(nt)
        model.forward(pool[0])
        t = time.time(); model.forward(pool[0]); t = time.time() - t
        if t < best[1]:
            best = (nt, t)
    torch.set_num_threads(best[0])
    n, t0, scores = 0, time.time(), []
    while n < len(pool) and (n == 0 or time.time() - t0 < budget_s):
        c, _ = torch_port.get_uncertainty(model, [pool[n]], augs, 21, bp=1.3, base_seed=0, positions=[positions[n]])
        scores.append(float(c[0]))
        n += 1
    dt = time.time() - t0
    used = torch.get_num_threads()
    torch.set_num_threads(default_threads)
    d = np.abs(np.asarray(scores) - np.asarray(gpu_scores[:n], np.float64))
    live = {"images_compared": n, "max_abs_consistency_diff": float(d.max()), "median_abs_consistency_diff": float(np.median(d)),
            "images_beyond_1e-4": int((d > 1e-4).sum()),
            "note": "measured in THIS run: the same pool images scored by the MI355X sweep and by the torch-CPU fp32 port (oneDNN "
                    "summation order, not the oracle's arithmetic contract); north_star's float tolerance is 1e-4"}
    return {"value": n / dt, "unit": "images/s", "cores": used, "images": n, "gpu_vs_cpu_port_live": live,
            "kind": "port (torch-CPU fp32 convs / linears; top-k, NMS, RoIAlign and post-processing in the OpenMP C oracle -- "
                    "stronger than the reference's pure-PyTorch CPU path)",
            "sample": "%d synthetic VOC-shaped image(s) x 4 views, batch-1 sequential torch-CPU fp32 forwards + python/scipy "
                      "scoring loop (oracle/torch_port.py), %.1f s; thread count chosen as the fastest of {T, T/2, T/4, T/8}" % (n, dt)}


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(d, cons, cls, picked):
    """--dump-outputs: what a caller of the timed path receives -- the per-image consistency scores, the cls_corr rows and the
    selected pool indices -- as DIR/<name>.npy in float64.  Above 64 MB in all, a fixed seeded sample of the per-image rows is
    written instead, with its row numbers (sample_rows.npy); the selected indices are always written whole."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    cons = np.asarray(cons, np.float64)
    cls = np.asarray(cls, np.float64).reshape(len(cons), -1)
    sel = np.asarray(picked, np.int64).astype(np.float64)
    row_bytes = 8 * (1 + cls.shape[1])
    room = DUMP_CAP_BYTES - 4096 - sel.nbytes                       # 4 KiB for the .npy headers
    if len(cons) * row_bytes > room:
        keep = max(1, room // (row_bytes + 8))
        rows = np.sort(np.random.RandomState(0).choice(len(cons), keep, replace=False))
        cons, cls = cons[rows], cls[rows]
        np.save(os.path.join(d, "sample_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(d, "consistency.npy"), cons)
    np.save(os.path.join(d, "cls_corr.npy"), cls)
    np.save(os.path.join(d, "selected_indices.npy"), sel)


def csrc_sha1():
    """Content hash of the kernel sources the library is built from (cald_amd/csrc/*.hip, *.h, Makefile), file names included.
    Stands where `git rev-parse HEAD:cald_amd/csrc` would: the GPU box receives a snapshot without .git."""
    h = hashlib.sha1()
    d = os.path.join(ROOT, "cald_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def latest_pmc():
    """HBM bytes per GEMM launch, achieved HBM GB/s and MFMA-busy fraction of the GEMM family from the rocprofv3 passes of
    this same command (tools/profile_gpu.sh -> tools/summarize_profile.py -> profiles/*_pmc.json; FETCH_SIZE x2 gfx950
    correction + WRITE_SIZE).  A process cannot attach rocprofv3 to itself, so the numbers come from a file -- but ONLY from a
    file that records the hash of the kernel sources it was measured on (`csrc_sha1`) and only when that hash is the running
    tree's: counters of other kernels are reported as null, never pasted beside live numbers."""
    here = csrc_sha1()
    try:
        for name in sorted(os.listdir(os.path.join(ROOT, "profiles")), reverse=True):
            if not name.endswith("_pmc.json"):
                continue
            d = json.load(open(os.path.join(ROOT, "profiles", name)))
            if d.get("csrc_sha1") == here and "conv_mfma" in d:
                c = d["conv_mfma"]
                return {"hbm_bytes_per_launch": c.get("hbm_bytes_per_launch"), "hbm_gbps": c.get("hbm_gbps"),
                        "mfma_busy": c.get("mfma_busy"), "source": "profiles/" + name, "csrc_sha1": here}
    except Exception:
        pass
    return {"hbm_bytes_per_launch": None, "hbm_gbps": None, "mfma_busy": None, "source": None, "csrc_sha1": here}


def parity_file():
    """Whole-pool parity against the torch-CPU fp32 path (tools/parity_full_pool.py -> profiles/parity_vs_independent_fp32_r*.json).
    Not measured in this run (the CPU path takes hours), so -- like the PMC counters -- it is reported only from a file that
    records the hash of exactly the running kernel sources; otherwise the field says which file is the latest and that it is stale."""
    here, latest = csrc_sha1(), None
    d = os.path.join(ROOT, "profiles")
    for name in sorted((f for f in os.listdir(d) if f.startswith("parity_vs_independent_fp32_r") and f.endswith(".json")), reverse=True):
        try:
            j = json.load(open(os.path.join(d, name)))
        except Exception:
            continue
        latest = latest or name
        if j.get("csrc_sha1") == here:
            return dict(j["summary"], from_file=True, measured_in_this_run=False, source="profiles/" + name, csrc_sha1=here)
    return {"from_file": False, "source": None, "csrc_sha1": here,
            "note": "no parity file was measured on exactly these kernel sources (latest: %s); figures of other kernels are not "
                    "pasted here" % (("profiles/" + latest) if latest else "none")}


def cfg4_f16x3_leg(local_rank, n=128):
    """BASELINE configs[4] on one GPU in ITS precision: Faster R-CNN ResNet-101 FPN, COCO-shaped synthetic images, 91 classes,
    min/max 800/1333, five augmentations (flip, ga, cut_out, smaller_resize, rotation: 6 views per image), precision f16x3 (the
    "fp16 MFMA path").  images/s of one cald_sweep call over n HBM-resident images, and the GEMM family's algorithmic FLOP rate
    (HIP events on the launch stream) against the dense fp16 MFMA peak.  Its parity gate is tests/test_gpu_parity.py::
    test_config4_full_size_f16x3_vs_exact (same workload against the exact mode)."""
    import ctypes as C
    import torch
    from cald_amd import _ffi, detector, sweep, synth
    augs = ["flip", "ga", "cut_out", "smaller_resize", "rotation"]
    sd = synth.pseudo_trained_frcnn(91, 101, seed=1)
    m = detector.fasterrcnn_resnet101_fpn_feature(num_classes=91, min_size=800, max_size=1333, precision="f16x3").to("cuda:%d" % local_rank)
    m.load_state_dict(sd)
    m.eval()
    dev = [torch.from_numpy(im).cuda() for im in synth.make_pool(n, "coco", 0)]
    pos = list(range(n))
    Bi = 64                                                  # 64 reference views, then 5 x 64 augmented views in forwards of <= 96
    sweep.sweep_device_images(m, dev[:Bi], pos[:Bi], augs, bp=1.3, base_seed=0, batch_images=Bi)      # warm-up: code objects, arena
    L, ctx = _ffi.lib(), detector.get_ctx(local_rank)
    _ffi.check(L.cald_profile_enable(ctx, 1))
    torch.cuda.synchronize(); t = time.time()
    cons, _ = sweep.sweep_device_images(m, dev, pos, augs, bp=1.3, base_seed=0, batch_images=Bi)
    torch.cuda.synchronize(); t = time.time() - t
    gm, gf, tot, nl = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    _ffi.check(L.cald_profile_read(ctx, C.byref(gm), C.byref(gf), C.byref(nl), C.byref(tot)))
    _ffi.check(L.cald_profile_enable(ctx, 0))
    del m
    torch.cuda.empty_cache()
    ach = gf.value / (gm.value * 1e-3) / 1e12 if gm.value > 0 else 0.0
    return {"workload": "BASELINE.json configs[4] (per GPU): Faster R-CNN ResNet-101 FPN, COCO-shaped synthetic images, 91 classes, min/max 800/1333, "
                        "5 augs (flip/ga/cut_out/smaller_resize/rotation = 6 views per image)",
            "headline": False, "value": n / t, "unit": "images/s", "images": n, "seconds": t, "sweep_batch_images": Bi,
            "dtype": "f16x3 (fp16 hi+lo split operands, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulate)",
            "scores_sha1": hashlib.sha1(cons.tobytes()).hexdigest(),
            "roofline": {"bound": "mfma", "achieved": ach, "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / F16_MFMA_PEAK_TFLOPS,
                         "launches": int(nl.value), "gemm_ms": gm.value,
                         "note": "algorithmic FLOPs counted once per product (three MFMAs issue per product: at most 1/3 of the pipe)"},
            "parity_gate": "tests/test_gpu_parity.py::test_config4_one_image_at_size_f16x3_vs_its_cpu_restatement (bit-identical to the CPU "
                           "restatement of the mode), ::test_config4_full_size_f16x3_vs_exact (statistics against the exact mode)"}


def config0_leg(model, sd, B, threads=None):
    """BASELINE configs[0] (the reference's CPU-runnable plumbing case: 200 synthetic VOC-shaped images, flip only) on the
    GPU, with the torch-CPU port (an fp32 path that does NOT share the arithmetic contract) scoring a bounded sample of
    the same images beside it -- a live measurement of 'KL/IoU floats within 1e-4 of the CPU path'."""
    import numpy as np
    import torch
    from cald_amd import synth, sweep
    from oracle import torch_port
    n, augs = 200, ["flip"]
    sizes = synth.pool_sizes(n, "voc", 0)
    imgs = [synth.synth_image(p, *sizes[p]) for p in range(n)]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    run = lambda: sweep.sweep_device_images(model, dev, list(range(n)), augs, bp=1.3, base_seed=0, batch_images=B)
    run()
    torch.cuda.synchronize(); t = time.time()
    cons, cls = run()
    torch.cuda.synchronize(); t = time.time() - t
    cpu = torch_port.TorchFRCNN(sd, 21, 50, 600, 1000)
    default_threads = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)         # the count cpu_baseline() found fastest on this host
    m, t0, ref = 0, time.time(), []
    while m < 8 and (m == 0 or time.time() - t0 < 8.0):
        c, _ = torch_port.get_uncertainty(cpu, [imgs[m]], augs, 21, bp=1.3, base_seed=0, positions=[m])
        ref.append(c[0]); m += 1
    tc = time.time() - t0
    torch.set_num_threads(default_threads)
    d = np.abs(np.asarray(ref) - cons[:m])
    return {"workload": "BASELINE.json configs[0]: Faster R-CNN ResNet-50 FPN, 200 synthetic VOC2012-shaped images, augs=['flip'] (2 views / image)",
            "headline": False, "gpu_images_per_s": n / t, "gpu_seconds": t,
            "scores_sha1": hashlib.sha1(np.ascontiguousarray(cons).tobytes()).hexdigest(),
            "cpu_port_images_per_s": m / tc, "cpu_port_sample": "%d of the 200 images, torch-CPU fp32 port (oracle/torch_port.py), %.1f s" % (m, tc),
            "max_abs_consistency_diff_gpu_vs_cpu_port": float(d.max()), "images_beyond_1e-4": int((d > 1e-4).sum()),
            "images_compared": m}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="steps of 64 pool images over the whole job; default: the full configs[1] pool (5 217 images = 82 steps) "
                         "in strong mode, 8 per GPU in weak mode")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch-images", type=int, default=None,
                    help="images per internal batch of the sweep; default: a step counts 64 images and the library batches the shard "
                         "in equal parts of <= 96 images")
    ap.add_argument("--scaling", default="strong", choices=["weak", "strong"],
                    help="strong (SURVEY 8d: fixed pool / wall time): K x 64 images in total, split over the N GPUs; "
                         "weak: K x 64 images per GPU (pool grows with N)")
    ap.add_argument("--comm", default="auto", choices=["auto", "cabi", "torch"],
                    help="who carries the one all-gather of the score rows (N > 1): cabi = cald_allgather_scores of the C ABI (RCCL, device "
                         "buffers, communicator bootstrapped over a TCP socket next to MASTER_PORT: no torch.distributed in the data path); "
                         "torch = torch.distributed.all_gather_into_tensor; auto = cabi when every rank has a GPU of its own, torch (gloo) when "
                         "ranks share a device (RCCL refuses two ranks on one GPU)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline (full pool, CPU baseline + configs[0], f16x3 mode, configs[4], training step) "
                         "and quote the committed parity file; a plain run only sets up, warms up and times the K steps")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path returned (consistency, cls_corr, selected indices) as DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-full-pool", action="store_true", help="skip the 5 217-image end-to-end run (N = 1 headline only)")
    ap.add_argument("--no-f16x3", action="store_true")
    ap.add_argument("--no-cfg4", action="store_true", help="skip the configs[4] leg (ResNet-101, COCO shapes, 5 augs, f16x3)")
    ap.add_argument("--no-train", action="store_true", help="skip the training-step leg (SURVEY 8f rank 4, informational)")
    ap.add_argument("--model", default="frcnn", choices=["frcnn", "frcnn101", "retinanet"],
                    help="frcnn = the headline workload (BASELINE configs[1]); others are informational runs of configs[2]/[4]")
    ap.add_argument("--shape", default="voc", choices=["voc", "coco"])
    ap.add_argument("--augs", default="FCD", help="letters of cald_train.py --augs (F C D R G S)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "f16x3"],
                    help="fp32 = exact (headline, bit-identical to the oracle); f16x3 = the opt-in split-fp16 matrix-pipe mode")
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ:      # plain `python bench.py --gpus N`: start the N ranks ourselves
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    args.batch_images_explicit = args.batch_images is not None
    B, Wm = (args.batch_images or 64), args.warmup
    full_default = args.steps is None and args.scaling == "strong"
    K = args.steps if args.steps is not None else ((FULL_POOL + B - 1) // B if full_default else 8)
    letters = {"F": "flip", "C": "cut_out", "D": "smaller_resize", "R": "rotation", "G": "ga", "S": "sp"}
    augs = [letters[ch] for ch in args.augs]
    ncls = 21 if args.shape == "voc" else 91
    mn, mx = (600, 1000) if args.shape == "voc" else (800, 1333)
    headline = (args.model == "frcnn" and args.shape == "voc" and args.augs == "FCD" and args.precision == "fp32")
    legs = headline and world == 1 and args.full       # the runs beyond the headline: only with --full
    do_full = legs and not args.no_full_pool and not full_default   # full_default: the headline IS the full pool
    full_scores = None

    # ---- the pool as files (host JPEG bytes): rank r owns pool positions p % world == r (rank-local inputs) ----
    from cald_amd import synth
    pool_total = world * K * B if args.scaling == "weak" else (FULL_POOL if full_default else K * B)
    n_warm = Wm * B
    total_needed = max(pool_total + world * n_warm, FULL_POOL if do_full else 0)
    sizes = synth.pool_sizes(total_needed, args.shape, 0)
    positions = list(range(rank, pool_total, world))                              # timed pool, this rank's shard
    warm_positions = list(range(pool_total + rank, pool_total + world * n_warm, world))
    blobs = make_jpeg_pool(positions, sizes)
    warm_blobs = make_jpeg_pool(warm_positions, sizes)
    full_blobs = None
    if do_full:
        have = dict(zip(positions, blobs))
        missing = [p for p in range(FULL_POOL) if p not in have]
        extra = dict(zip(missing, make_jpeg_pool(missing, sizes)))
        full_blobs = [have[p] if p in have else extra[p] for p in range(FULL_POOL)]

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU fallback for the product path"
    # N ranks on fewer than N visible GPUs (a 1-GPU box): the ranks share the device(s) and the collective goes over gloo,
    # because RCCL refuses two ranks on one device (tools/nccl_same_gpu_probe.py).  CALD_BENCH_SHARE_GPU=1 forces that.
    ndev = torch.cuda.device_count()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    share = world > 1 and (os.environ.get("CALD_BENCH_SHARE_GPU") == "1" or ndev < local_world)
    if share:
        local_rank = local_rank % ndev
    torch.cuda.set_device(local_rank)
    dist = None
    backend = "none"
    if world > 1:
        import torch.distributed as dist
        backend = "gloo" if share else "nccl"
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    coll_dev = torch.device("cpu") if (share or world == 1) else torch.device("cuda", local_rank)
    use_cabi = world > 1 and (args.comm == "cabi" or (args.comm == "auto" and not share))
    cabi_comm, cabi_info = None, None

    from cald_amd import _ffi, detector, sweep
    from cald_amd.pool import DevicePool
    if args.model == "retinanet":
        sd = synth.pseudo_trained_retinanet(ncls, 50, seed=0)
        model = detector.retinanet_resnet50_fpn_cal(num_classes=ncls, min_size=mn, max_size=mx, precision=args.precision)
    else:
        depth = 101 if args.model == "frcnn101" else 50
        sd = synth.pseudo_trained_frcnn(ncls, depth, seed=0)
        model = (detector.fasterrcnn_resnet101_fpn_feature if depth == 101 else detector.fasterrcnn_resnet50_fpn_feature)(
            num_classes=ncls, min_size=mn, max_size=mx, precision=args.precision)
    model = model.to("cuda:%d" % local_rank)
    model.load_state_dict(sd)
    model.eval()
    cabi_note = None
    if use_cabi:
        # the C ABI's own communicator (cald_comm_init_rank): one per process, on the context's device and stream.  Every step is agreed on
        # by all ranks through the launcher's process group, so that a rank that cannot bootstrap (a port taken, RCCL missing) sends the whole
        # job to the torch.distributed gather instead of leaving its peers in a collective alone; the JSON line says which path ran.
        from cald_amd.comm import RcclComm
        import ctypes as C_

        def all_ok(ok):
            t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=coll_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(int(t.item()))
        uid, err = None, None
        try:
            uid = exchange_id_over_tcp(rank, world, RcclComm.unique_id() if rank == 0 else None, timeout_s=60.0)
            bootstrap = "128-byte id over TCP (MASTER_PORT + 29)"
        except Exception as e:                       # noqa: BLE001 -- any failure here must not strand the other ranks
            err = "tcp bootstrap: %r" % (e,)
        if not all_ok(uid is not None):
            box = [None]
            if rank == 0:
                try:
                    box = [RcclComm.unique_id()]
                except Exception as e:               # noqa: BLE001
                    err = "ncclGetUniqueId: %r" % (e,)
            dist.broadcast_object_list(box, src=0)
            uid, bootstrap = box[0], "128-byte id through the launcher's process group (the TCP side channel failed: %s)" % err
        if all_ok(uid is not None):
            try:
                cabi_comm = RcclComm.init_rank(uid, world, rank, device=local_rank)
                w_, r_ = C_.c_int(), C_.c_int()
                _ffi.check(_ffi.lib().cald_comm_info(cabi_comm.handle, C_.byref(w_), C_.byref(r_)))
                cabi_info = (w_.value, r_.value)
                assert cabi_info == (world, rank), cabi_info
            except Exception as e:                   # noqa: BLE001
                err, cabi_comm = "cald_comm_init_rank: %r" % (e,), None
        if not all_ok(cabi_comm is not None):
            if cabi_comm is not None:
                cabi_comm.close()
            cabi_comm, cabi_note = None, "C-ABI collective unavailable on some rank (%s): torch.distributed gathered the rows" % (err or "a peer failed")
        else:
            wp = sweep.shard_positions(world * 3, rank, world)            # warm-up on a 3-rows-per-rank pool: RCCL's first collective builds its rings
            cabi_comm.allgather_scores(wp, np.zeros(len(wp)), np.zeros((len(wp), ncls - 1)), world * 3)
    labeled = synthetic_labeled_set(500, ncls, 0)
    budget = max(1, min(FULL_BUDGET, int(round(FULL_BUDGET * pool_total / float(FULL_POOL)))))

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def balanced(n, cap=96):
        """Images per internal batch of one cald_sweep call: the shard split into equal batches of at most `cap` images, so that the
        reference forward (B views) and the augmented forwards (3 B views in forwards of <= 96) all run near the 96-view size that
        fills whole rounds of workgroup slots -- a 160-image strong-scaling shard runs 2 x 80, not 64 + 64 + 32 (or 54 + 53 + 53)."""
        if args.batch_images_explicit:
            return B
        cap = int(os.environ.get("CALD_BENCH_BATCH_CAP", cap))      # e.g. 40 when eight ranks rehearse on ONE GPU (eight arenas in one HBM)
        if os.environ.get("CALD_BENCH_BALANCE", "equal") == "cap":   # batches of exactly `cap` images and one remainder batch
            return max(1, min(cap, n))
        return max(1, -(-n // max(1, -(-n // cap))))

    Bi = balanced(len(positions))                  # the timed call's internal batch size; the warm-up runs with the same one

    def sweep_batch(pool, pos, lo, hi):
        return sweep.sweep_device_images(model, [pool[i] for i in range(lo, hi)], pos[lo:hi], augs, bp=1.3, base_seed=0, batch_images=Bi)

    # ---- warm-up: decode path, code objects, workspace arena, W untimed steps ----
    warm_pool = DevicePool.from_jpeg_bytes(warm_blobs if warm_blobs else blobs[:B])
    wpos = warm_positions if warm_blobs else positions[:B]
    sweep_batch(warm_pool, wpos, 0, len(warm_pool))       # W x 64 untimed images through the same call shape as the timed region
    del warm_pool

    # ---- host JPEG bytes -> HBM-resident uint8 pool (decode on the GPU), timed on its own ----
    barrier()
    t0 = time.time()
    dev_pool = DevicePool.from_jpeg_bytes(blobs)
    torch.cuda.synchronize()
    t_decode = time.time() - t0

    L, ctx = _ffi.lib(), detector.get_ctx(local_rank)
    _ffi.check(L.cald_profile_enable(ctx, 1))     # HIP events around every conv/linear launch on the launch stream
    n_local = len(positions)
    steps_local = (n_local + B - 1) // B          # == K for weak scaling; K / N (rounded up) for strong scaling
    # equal-sized batches (strong scaling leaves e.g. 160 images per rank: 54 + 53 + 53, not 64 + 64 + 32)
    # ONE cald_sweep call over the rank's shard: the library walks it in equal batches and keeps two in flight (the reference forward
    # of batch k + 1 runs while the host builds batch k's augmented views; the stream never waits for the host)
    barrier()
    t0 = time.time()
    if n_local:
        cons, cls = sweep_batch(dev_pool, positions, 0, n_local)
    else:
        cons, cls = np.zeros(0), np.zeros((0, ncls - 1))
    t_local = time.time() - t0                    # this rank's own shard scored (sweep_batch returns host arrays: synchronous)
    if world > 1:   # the one RCCL all-gather of the (consistency, cls_corr) rows of the WHOLE timed pool
        cons, cls = (cabi_comm.allgather_scores(positions, cons, cls, pool_total) if cabi_comm is not None else
                     sweep.allgather_scores(positions, cons, cls, pool_total))
    picked = sweep.select(list(cons), [cls[i] for i in range(cls.shape[0])], labeled, budget=budget, mr=1.2)   # every rank, host
    barrier()
    dt = time.time() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, cons, cls, picked)
    # who took part: every rank's device identity, shard size and own sweep time, gathered through the SAME process group
    # (RCCL when `backend` is nccl) -- outside the timed region
    props = torch.cuda.get_device_properties(local_rank)
    ident = hashlib.sha1(("%s|%s" % (getattr(props, "uuid", ""), torch.cuda.get_device_name(local_rank))).encode()).digest()[:8]
    try:
        bus = int(getattr(props, "pci_bus_id", -1))
    except Exception:
        bus = -1
    row = torch.tensor([float(rank), float(local_rank), float(bus), float(int.from_bytes(ident[:6], "big")),
                        float(n_local), t_local, dt, t_decode], dtype=torch.float64, device=coll_dev)
    rows = row[None]
    if world > 1:
        rows = torch.empty(world * row.numel(), dtype=torch.float64, device=coll_dev)
        dist.all_gather_into_tensor(rows, row)
    rows = rows.cpu().numpy().reshape(world, -1)
    dt, t_decode = float(rows[:, 6].max()), float(rows[:, 7].max())     # max over ranks
    uuid_s = str(getattr(props, "uuid", ""))
    import ctypes as C
    gm, gf, tot, mean_r = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    nl, nviews = C.c_int64(), C.c_int64()
    _ffi.check(L.cald_profile_read(ctx, C.byref(gm), C.byref(gf), C.byref(nl), C.byref(tot)))
    _ffi.check(L.cald_profile_roi_rows(ctx, C.byref(mean_r), C.byref(nviews)))
    look_ms, look_fl = C.c_double(), C.c_double(); sel_frac = (C.c_double * 2)()
    worst_ratio, pruned_fl = C.c_double(), C.c_double()
    _ffi.check(L.cald_profile_prune(ctx, C.byref(look_ms), C.byref(look_fl), sel_frac, C.byref(worst_ratio), C.byref(pruned_fl)))
    if os.environ.get("CALD_PROFILE_DUMP"):
        _ffi.check(L.cald_profile_dump(ctx, os.environ["CALD_PROFILE_DUMP"].encode()))
    _ffi.check(L.cald_profile_enable(ctx, 0))

    if rank == 0:
        pmc = latest_pmc()
        achieved = gf.value / (gm.value * 1e-3) / 1e12 if gm.value > 0 else 0.0
        peak = {"fp32": F32_MFMA_PEAK_TFLOPS, "f16x3": F16_MFMA_PEAK_TFLOPS}[args.precision]
        out = {
            "metric": "unlabeled images scored/sec (CALD consistency sweep)", "value": pool_total / dt, "unit": "images/s",
            "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": dt / max(1, K) * 1e3, "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None,
            "dtype": {"fp32": "f32", "f16x3": "f16x3 (fp16 hi+lo split operands, fp32 accumulate)"}[args.precision],
            "data": "synthetic",
            "config": {"workload": ("BASELINE.json configs[1]: Faster R-CNN ResNet-50 FPN, VOC2012-shaped synthetic pool (baseline JPEG files), "
                                    "3 augs (flip/cut_out/smaller_resize), 21 classes, min/max 600/1000, seeded pseudo-trained weights")
                       if headline else "informational: model=%s shape=%s augs=%s classes=%d min/max %d/%d precision=%s" % (args.model, args.shape, args.augs, ncls, mn, mx, args.precision),
                       "images_per_step": B, "images_per_step_note": "a step counts 64 pool images; weak scaling: per GPU; strong scaling: over the whole job",
                       "sweep_batch_images": Bi, "sweep_calls": 1,
                       "views_per_image": 1 + len(sweep.expand_augs(augs)), "pool_images": pool_total,
                       "timed_region": "HBM-resident decoded pool -> K sweep steps -> all-gather (N>1) -> argsort + cls_kldiv -> selected indices",
                       "selection_budget": budget, "n_selected": int(len(picked)),
                       "selected_sha1": hashlib.sha1(np.asarray(picked, np.int64).tobytes()).hexdigest(),
                       "parallelism": "pool sharded by position (rank-local inputs), dp%d" % world,
                       "steps_per_rank": steps_local},
            "rccl": {"backend": backend, "world_size": world, "ranks_seen": int(rows.shape[0]), "visible_gpus": ndev,
                     "shared_gpu": bool(share),
                     "cabi": ({"world_size": cabi_info[0], "rank0": cabi_info[1], "bootstrap": bootstrap} if cabi_comm is not None else
                              ({"error": cabi_note} if cabi_note else None)),
                     "collective": ("cald_allgather_scores (C ABI: RCCL on the context's stream, device buffers, communicator from cald_comm_init_rank)" if cabi_comm is not None else
                                    "all_gather_into_tensor over RCCL (device buffers)" if backend == "nccl" else
                                    "all_gather_into_tensor over gloo: %d ranks on %d visible GPU(s), RCCL refuses two ranks on one device" % (world, ndev)
                                    if backend == "gloo" else "none (one rank)"),
                     "per_rank": [{"rank": int(r[0]), "device": int(r[1]), "pci_bus": int(r[2]), "device_id_hash": "%012x" % int(r[3]),
                                   "images": int(r[4]), "images_per_s": (r[4] / r[5]) if r[5] > 0 else None, "sweep_s": r[5]}
                                  for r in rows],
                     "distinct_devices": len({(int(r[2]), int(r[3])) for r in rows}), "rank0_device_uuid": uuid_s,
                     "host_cpus_usable": usable_cpus()},
            "from_host_jpeg_bytes": {"value": pool_total / (dt + t_decode), "unit": "images/s", "decode_and_h2d_s": t_decode,
                                     "note": "same pool, JPEG decode on the GPU + H2D included (max over ranks); never `value`"},
            "roofline": {"bound": "mfma",
                         "kernel": {"fp32": "conv_p4_kernel + conv_mfma_f32_kernel (implicit-GEMM conv + linear, v_mfma_f32_32x32x2_f32)",
                                    "f16x3": "conv_h3_kernel / conv_h4_kernel (3 x v_mfma_f32_32x32x16_f16 per product; algorithmic flops counted once: at most 1/3 of the pipe's peak; measured power ceiling on random operands ~0.15, profiles/r4_f16x3_zero_vs_random_operands.txt) + exact kernels for uncovered shapes"}[args.precision],
                         "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                         "frac": achieved / peak, "traffic": pmc["hbm_bytes_per_launch"] if args.precision == "fp32" else None,
                         "hbm_gbps": pmc["hbm_gbps"] if args.precision == "fp32" else None,
                         "mfma_busy": pmc["mfma_busy"] if args.precision == "fp32" else None,
                         "counters": {"from_file": pmc["source"] is not None, "source": pmc["source"], "csrc_sha1": pmc["csrc_sha1"],
                                      "note": "traffic / hbm_gbps / mfma_busy: the committed rocprofv3 PMC summary of this command, used only when "
                                              "it was measured on exactly these kernel sources (csrc_sha1 recorded in the file), else null; "
                                              "achieved / frac / launches are measured live (HIP events)"},
                         "launches": int(nl.value), "avg_launch_ms": gm.value / max(1, nl.value),
                         "gemm_ms_per_step": gm.value / max(1, steps_local), "algorithmic_gflop_per_launch": gf.value / max(1, nl.value) / 1e9,
                         "roi_rows_per_view_measured": mean_r.value,
                         "rpn_prune": None if look_ms.value <= 0 else {
                             "what": "certified RPN pruning of the exact sweep (cald_amd/csrc/rpn_prune.hip): the RPN head of P2 / P3 is evaluated exactly only "
                                     "at the pixels that can hold a top-1000 anchor, found by a split-fp16 look-ahead with an error bound; detections bit-identical",
                             "lookahead_ms_per_step": look_ms.value / max(1, steps_local), "lookahead_tflops_eq": look_fl.value / max(look_ms.value, 1e-9) / 1e9,
                             "pixels_recomputed_exactly": {"P2": sel_frac[0], "P3": sel_frac[1]},
                             "worst_observed_error_over_bound": worst_ratio.value,
                             "note": "achieved / frac / launches above count the fp32 kernels only, the gathered launches on their selected rows; "
                                     "the look-ahead launches (fp16 matrix pipe) are booked here"},
                         "algorithmic": None if look_ms.value <= 0 else {
                             "tflops": (gf.value + pruned_fl.value) / ((gm.value + look_ms.value) * 1e-3) / 1e12,
                             "frac": (gf.value + pruned_fl.value) / ((gm.value + look_ms.value) * 1e-3) / 1e12 / peak,
                             "note": "the dense graph's fp32 FLOPs (executed + pruned away) / (fp32 kernel time + look-ahead time): the task contract's "
                                     "'algorithmic FLOPs / launch duration'; `frac` above is the stricter one -- only FLOPs the fp32 kernels really execute"},
                         "reference_algorithmic_tflops": (0.8416e12 if headline else 0.0) * pool_total / dt / 1e12 if headline else None,
                         "note": "rank 0's launches, HIP events on the launch stream; RoI-head FLOPs counted on the measured proposal rows; "
                                 "reference_algorithmic_tflops = images/s x 0.84 TFLOP per image (4 views x 105.2 GMAC, SURVEY 8d), what the reference's dense graph would cost"},
        }
        if do_full:
            # BASELINE configs[1] at its full size, one clock around everything: host JPEG bytes -> decode on the GPU ->
            # sweep -> argsort + cls_kldiv (budget 500, mr 1.2) -> indices
            del dev_pool
            torch.cuda.synchronize(); tf = time.time()
            fp = DevicePool.from_jpeg_bytes(full_blobs)
            unc, ccs = sweep.get_uncertainty(model, fp.loader(), augs, ncls, bp=1.3, base_seed=0, batch_images=96)
            sel = sweep.select(unc, ccs, labeled, budget=FULL_BUDGET, mr=1.2)
            torch.cuda.synchronize(); tf = time.time() - tf
            u = np.asarray(unc)
            out["full_pool"] = {"value": FULL_POOL / tf, "unit": "images/s", "pool_images": FULL_POOL, "seconds": tf, "budget": FULL_BUDGET,
                                "n_selected": int(len(sel)), "selected_sha1": hashlib.sha1(np.asarray(sel, np.int64).tobytes()).hexdigest(),
                                "zero_score_images": int((u == 0).sum()),
                                "timed_region": "host JPEG bytes -> GPU decode -> get_uncertainty -> argsort + cls_kldiv -> 500 indices"}
            dev_pool = fp
            full_scores = (u, np.stack(ccs))
        if legs and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(sd, blobs, augs, positions, cons)
            out["cpu_baseline"]["host_cpus"] = os.cpu_count()
            out["cpu_baseline"]["host_cpus_usable"] = usable_cpus()
            out["config0_cpu_plumbing"] = config0_leg(model, sd, B, threads=out["cpu_baseline"]["cores"])
        if legs and not args.no_f16x3:
            # informational second line, NOT the headline: the opt-in split-fp16 MFMA mode (BASELINE configs[4]'s "fp16 MFMA path")
            # on the SAME timed pool, with its parity statement measured in this run: every image the exact mode just scored is
            # scored again in f16x3 and the two selections are compared
            fast = (detector.fasterrcnn_resnet50_fpn_feature(num_classes=ncls, min_size=mn, max_size=mx, precision="f16x3")
                    .to("cuda:%d" % local_rank))
            fast.load_state_dict(sd)
            fast.eval()
            nb = len(dev_pool)                          # do_full: the whole configs[1] pool (5 217 images), else the timed pool
            imgs = [dev_pool[i] for i in range(nb)]
            pos_f = list(range(nb)) if do_full else positions[:nb]
            run = lambda mdl: sweep.sweep_device_images(mdl, imgs, pos_f, augs, bp=1.3, base_seed=0, batch_images=96)
            sweep.sweep_device_images(fast, imgs[:192], pos_f[:192], augs, bp=1.3, base_seed=0, batch_images=96)   # warm-up
            torch.cuda.synchronize(); tf = time.time()
            fc, fk = run(fast)
            torch.cuda.synchronize(); tf = time.time() - tf
            ec, ek = full_scores if do_full else (cons[:nb], cls[:nb])       # the exact mode's scores of this run's own sweep
            d = np.abs(fc - ec)
            bud = max(1, min(FULL_BUDGET, int(round(FULL_BUDGET * nb / float(FULL_POOL)))))
            sel_e = sweep.select(list(ec), [ek[i] for i in range(nb)], labeled, budget=bud, mr=1.2)
            sel_f = sweep.select(list(fc), [fk[i] for i in range(nb)], labeled, budget=bud, mr=1.2)
            out["f16x3_mode"] = {"value": nb / tf, "unit": "images/s", "dtype": "fp16 hi+lo split operands, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulate",
                                 "headline": False, "measured_in_this_run": True, "images_compared": nb,
                                 "max_abs_consistency_diff_vs_exact": float(d.max()), "median_abs_consistency_diff_vs_exact": float(np.median(d)),
                                 "images_beyond_1e-4_vs_exact": int((d > 1e-4).sum()),
                                 "selection_budget": bud, "selected_same_set_vs_exact": int(len(set(map(int, sel_e)) & set(map(int, sel_f)))),
                                 "selected_total": int(len(sel_e)), "selected_identical_order": bool(list(map(int, sel_e)) == list(map(int, sel_f))),
                                 "selection_vs_its_own_cpu_restatement": "identical (bit for bit): oracle/f16x3_oracle.c + mfma_f16_model.h restate the mode down to "
                                         "v_mfma_f32_32x32x16_f16; tests/test_gpu_parity.py::test_sweep_f16x3_matches_oracle, "
                                         "::test_config4_one_image_at_size_f16x3_vs_its_cpu_restatement, ::test_mfma_f16_model_equals_the_hardware",
                                 "note": "the differences above are against the EXACT mode, i.e. between two arithmetics: a thresholded pipeline flips a "
                                         "borderline detection on ~1 % of these pseudo-trained images under ANY change of rounding -- the exact mode against "
                                         "an independent fp32 path does the same (parity_vs_independent_fp32); on a detector trained by this repo "
                                         "0 of 1 024 images move by more than 1e-5 (profiles/r6_trained_weights.json)"}
            del fast
        if legs and not args.no_cfg4:
            out["cfg4_f16x3"] = cfg4_f16x3_leg(local_rank)
        if legs and not args.no_train:
            # informational, NOT the headline: one training step of the same detector, cald_train.py's defaults
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_train
            del model
            torch.cuda.empty_cache()
            out["training_step"] = dict(bench_train.measure(batch=4, steps=10, warmup=3), headline=False)
        if args.full:
            out["parity_vs_independent_fp32"] = parity_file()
        print(json.dumps(out))
    if cabi_comm is not None:
        cabi_comm.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
