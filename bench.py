#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X path tracer.

Metric (BASELINE.json): Mpaths/s at 1920x1080, 4 bounces (config C2:
cornellbox, 64 spp, L = 4, diffuse).  One "step" = one complete C2 render:
reset + 64 frames (1 spp each; one launch of the hot kernel per 64-frame batch) on the tiles this
rank owns, plus — for N > 1 — the single RCCL exchange of the accumulation
image to rank 0, done by libmrt itself (mrt_renderer_exchange: a gather of
the packed owned tiles, overlapped with the next step's draw; or an in-place
SUM reduce).  value = paths of all ranks / max-over-ranks step time (strong
scaling: the frame is split into 64x64 tiles, tile t on rank t % N).
torch is used only as the CPU control plane for N > 1 (gloo: the RCCL unique
id broadcast, barriers and the max over ranks); no torch GPU state exists.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--config c1|c2|c3|c3g|c4|c5]
                       [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the result line
(value, ms_per_step, the hot kernel's roofline from the timed steps' own
counters).  --dump-outputs DIR also writes the image of the last timed step
(what a caller of the path reads back, mrt_renderer_read_image) as
DIR/image.npy.  --full adds everything that takes runs of its own: the
sustained window after the timed steps, the CPU oracle baseline with the image
parity legs (fast and precise build), the host noise-table timing and c2i's
bitwise check against the batched render.
N > 1: one process per GPU.  Under torch.distributed.run (WORLD_SIZE set) each
process is one rank; without it, bench.py starts the N ranks itself (children
with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, before any HIP call),
prints rank 0's line and fails if any rank fails.  --sweep-gpus 1,2,4,8 runs
one such job per N and prints one line each (e.g. --config c5 on one node).
--shard-of S (N = 1 only): render only rank 0's tiles of an S-way split —
one GPU's share of a multi-GPU job, value = that share's paths/s (diagnostic).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "metal-renderer_amd"))

METRIC = "Mpaths/s at 1920×1080, 4 bounces; achieved HBM GB/s vs peak; 1/2/4/8-GPU scaling"
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# VALU issue roof: 256 CUs x 4 SIMDs, a wave64 VALU instruction issues over 2
# cycles (32 lanes/cycle per SIMD, MI355X_MICROARCH.md), at the 2.4-GHz peak
# engine clock = 78.6 T lane-ops/s (the FP32 vector peak 157.3 TFLOP/s / 2)
VALU_PEAK_TLANE = 1024 * 32 * 2.4e9 / 1e12
B_PATH, B_BOUNCE = 112, 312    # algorithmic bytes per path / per active ray-bounce

CONFIGS = {
    # BASELINE.json configs[0]: the reference's CPU-runnable plumbing case (also on the GPU)
    "c1": dict(workload="C1 cornellbox 256x256 1spp L=1", scene="cornellbox", mtl=None,
               width=256, height=256, spp=1, L=1, procedural=0),
    # BASELINE.json configs[1] — the metric's config
    "c2": dict(workload="C2 cornellbox 1920x1080 64spp L=4 (diffuse BSDF)", scene="cornellbox", mtl=None,
               width=1920, height=1080, spp=64, L=4, procedural=0),
    # configs[2]: CornellBox-Water-plastic (plastic + mirror + water), 256 spp, L = 8
    "c3": dict(workload="C3 CornellBox-Water-plastic 1920x1080 256spp L=8", scene="CornellBox-Water-plastic",
               mtl=None, width=1920, height=1080, spp=256, L=8, procedural=0),
    # configs[2] with the generated "glass" variant: the water
    # becomes a dielectric (Ks 0 0 +1.33333), so diffuse walls, the mirror
    # sphere, the plastic sphere and the dielectric water exercise all 4 BSDFs
    "c3g": dict(workload="C3 CornellBox-Water-plastic + glass water 1920x1080 256spp L=8 (all 4 BSDFs)",
                scene="CornellBox-Water-plastic", mtl="glass-water", width=1920, height=1080, spp=256, L=8,
                procedural=0),
    # configs[3]: 1M-triangle procedural mesh in the cornellbox shell, 64 spp, L = 4
    "c4": dict(workload="C4 1M-triangle procedural mesh 1920x1080 64spp L=4", scene="cornellbox", mtl=None,
               width=1920, height=1080, spp=64, L=4, procedural=1 << 20),
    # C2 at MAX_PATH_LENGTH 5: north_star's "primary ray + 4 bounces" reading
    # of the headline (C2's L = 4 is the primary ray + 3 bounces as
    # renderer/Renderer.mm:517 loops MAX_PATH_LENGTH, Raytracing.h:23)
    "c2l5": dict(workload="C2 at L=5: cornellbox 1920x1080 64spp, primary ray + 4 bounces (diffuse BSDF)",
                 scene="cornellbox", mtl=None, width=1920, height=1080, spp=64, L=5, procedural=0),
    # C2 at the reference's own cadence: one drawInMTKView: (1 spp) per call
    # (renderer/Renderer.mm:587-638) — a step is 64 calls of mrt_renderer_draw,
    # progressive (no reset between steps, so every step renders new frames and
    # their noise tables are generated inside the timed region)
    "c2i": dict(workload="C2 at the per-frame cadence: 64 calls of mrt_renderer_draw (1 spp each) per step, "
                         "progressive, noise generated inside the timed region", scene="cornellbox", mtl=None,
                width=1920, height=1080, spp=64, L=4, procedural=0, cadence="frame"),
    # configs[4]: C4's scene at 4K, 256 spp, L = 8 — the 8-GPU configuration
    # (one GPU's share is measured with --shard-of 8)
    "c5": dict(workload="C5 1M-triangle procedural mesh 3840x2160 256spp L=8", scene="cornellbox", mtl=None,
               width=3840, height=2160, spp=256, L=8, procedural=1 << 20),
}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=None,
                   help="timed steps (default: 100 for c2 / c2l5, whose step is ~12 ms, so the timed region is "
                        "over a second; 5 otherwise)")
    p.add_argument("--warmup", type=int, default=None, help="untimed steps (default: 5 for c2 / c2l5, 1 otherwise)")
    p.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    p.add_argument("--max-path-length", type=int, default=0,
                   help="override the config's MAX_PATH_LENGTH (e.g. 5 = primary ray + 4 bounces)")
    p.add_argument("--precise", action="store_true", help="time the parity build instead of the fast build")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run what the headline value does not need: the --sustain "
                        "window, the CPU oracle baseline + image parity legs, the host noise-table timing and "
                        "c2i's bitwise image check (each still has its own switch below)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="write the image of the last timed step (rank 0's, as mrt_renderer_read_image returns it) "
                        "to DIR/image.npy (float32; above 64 MB a fixed seeded sample of its pixels)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU oracle baseline / parity legs")
    p.add_argument("--bvh", default="sah", choices=["sah", "lbvh", "ploc"],
                   help="BVH builder: host binned SAH (default), device LBVH or device PLOC")
    p.add_argument("--cpu-frames", type=int, default=0,
                   help="frames of the workload timed on the CPU oracle (default: all spp frames for C2, 8 otherwise)")
    p.add_argument("--pmc", default=None, help="JSON with the PMC counts per hot-kernel launch (profiles/pmc_<config>.json)")
    p.add_argument("--shard-of", type=int, default=0,
                   help="N=1 only: time rank 0's tiles of an S-way tile split (one GPU's share)")
    p.add_argument("--shard-rank", type=int, default=0,
                   help="with --shard-of: which rank's tiles to render (default 0)")
    p.add_argument("--no-kernel-timing", action="store_true",
                   help="no HIP events around the hot kernel's launches (diagnostic: the events' own cost)")
    p.add_argument("--exchange", default="gather", choices=["gather", "reduce"],
                   help="N>1 image exchange: RCCL gather of packed owned tiles (default) or SUM reduce of the image")
    p.add_argument("--no-overlap", action="store_true",
                   help="N > 1: exchange inside each step instead of overlapping it with the next step's draw")
    p.add_argument("--check-image", action="store_true",
                   help="N>1: rank 0 renders the frame alone afterwards and asserts the exchanged image is bitwise equal")
    p.add_argument("--check-image-tolerance", action="store_true",
                   help="with --check-image: accept <= 1e-5 of the pixels differing, each within rel-L2 1e-3 "
                        "(the differing count is reported either way)")
    p.add_argument("--exchange-backend", default="rccl", choices=["rccl", "host"],
                   help="rccl: libmrt's RCCL collective (one process per GPU); host: packed tiles through host "
                        "memory and a gloo gather (rehearsal of the N>1 path with several ranks on one GPU)")
    p.add_argument("--sustain", type=float, default=10.0,
                   help="with --full, N=1 batched configs: after the timed steps, keep stepping for this many seconds "
                        "and report the sustained rate beside the line (0 = off; not the headline value)")
    p.add_argument("--no-image-check", action="store_true",
                   help="c2i: skip the bitwise check of the timed image against draw_n (profiling passes)")
    p.add_argument("--sweep-gpus", default="",
                   help="comma-separated GPU counts (e.g. 1,2,4,8): one job per N, one JSON line each")
    p.add_argument("--rank-timeout", type=float, default=1800.0,
                   help="self-launched ranks: seconds before a job whose ranks have not all exited is killed")
    args = p.parse_args()
    long_default = args.config in ("c2", "c2l5")
    if args.steps is None:
        args.steps = 100 if long_default else 5
    if args.warmup is None:
        args.warmup = 5 if long_default else 1
    return args


def _child_argv(n):
    """This command line for a self-launched job of n ranks (--gpus n, no sweep)."""
    out, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
            continue
        if a in ("--gpus", "--sweep-gpus"):
            skip = True
            continue
        if a.startswith("--gpus=") or a.startswith("--sweep-gpus="):
            continue
        out.append(a)
    return [sys.executable, os.path.abspath(__file__)] + out + ["--gpus", str(n)]


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args):
    """Start each job's ranks as child processes (this process never touches
    the GPU); rank 0 prints the JSON line.  Returns the first non-zero exit
    status, after stopping the job's other ranks."""
    import subprocess
    counts = [int(x) for x in args.sweep_gpus.split(",") if x.strip()] if args.sweep_gpus else [args.gpus]
    for n in counts:
        port = _free_port()
        procs = []
        for rank in range(n):
            env = dict(os.environ)
            if n > 1:
                env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                           GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            procs.append(subprocess.Popen(_child_argv(n), env=env))
        t_end = time.time() + args.rank_timeout
        failed = 0
        while any(p.poll() is None for p in procs):
            bad = [p.returncode for p in procs if p.returncode not in (None, 0)]
            if bad or time.time() > t_end:
                failed = bad[0] if bad else 124
                for p in procs:   # the ranks this process started (exact PIDs)
                    if p.poll() is None:
                        p.terminate()
                for p in procs:
                    try:
                        p.wait(timeout=30)
                    except subprocess.TimeoutExpired:
                        p.kill()
                break
            time.sleep(0.2)
        failed = failed or next((p.returncode for p in procs if p.returncode), 0)
        if failed:
            print(f"bench.py: a rank of the {n}-GPU job failed (exit {failed})", file=sys.stderr, flush=True)
            return failed
    return 0


def resolve_mtl(cfg):
    """Material override of a config: None (the OBJ's own mtllib) or a
    generated variant written next to the run's outputs."""
    if cfg["mtl"] != "glass-water":
        return cfg["mtl"]
    import tempfile
    import mrt
    src = open(mrt.scene_path(cfg["scene"])[:-4] + ".mtl").read()
    out = os.path.join(tempfile.gettempdir(), f"mrt-{os.getpid()}-glass-water.mtl")
    with open(out, "w") as f:
        f.write(src.replace("Ks 0.0 0.0 -1.33333", "Ks 0.0 0.0 1.33333"))
    return out


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def lib_md5(path):
    import hashlib
    h = hashlib.md5()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def affinity_cpus():
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def host_threads():
    """Worker threads of the CPU baseline: the CPUs this process may run on
    (affinity mask), capped by the worker-pool size the GPU pool sets for one
    GPU's share of a shared 8-GPU host (OMP_NUM_THREADS=16 there, with the
    rule to size worker pools to that share; the affinity mask and
    os.cpu_count() report the whole 256-CPU machine).  Without the variable
    (e.g. a dedicated host) every CPU of the affinity mask is used."""
    n = affinity_cpus()
    cap = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return max(1, min(n, cap) if cap > 0 else n)


def cpu_baseline(cfg, frames):
    """The CPU oracle (scalar C++ restatement of the path, oracle/) timed on
    this host on a bounded sample of the same workload, its
    nearest hits through a binned-SAH BVH (oracle ORC_BVH: the same answers
    as its brute force, tests/test_oracle.py; its culling slack, 2^-6 of the
    hit's t, is independent of the kernels' 2^-11) — "same
    BVH", not brute force.
    C2 runs in full (all `frames` = spp frames of the whole image) on every
    CPU of the process's share, and 2 frames on one thread give the scalar
    rate.  Other scenes run one frame of a row band sized from a pilot band to
    ~10 s on all threads and ~10 s on one.
    Returns (baseline dict, oracle image, pixel mask, frames) — the image is
    kept for the parity check of the GPU render (main)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import oracle  # test/baseline infrastructure only (see oracle/mrt_oracle.cpp header)
    import mrt
    if not os.path.exists(oracle.LIB_PATH):
        oracle.build()
    threads = host_threads()
    if cfg["procedural"]:
        # the product's flattened scene (the seeded procedural mesh is built by
        # libmrt's scene import; the oracle builds its BVH over the same buffers)
        e = mrt.Scene(cfg["scene"], resolve_mtl(cfg), procedural_triangles=cfg["procedural"], device=-1).export()
        sc = oracle.OracleScene.from_arrays(e["vertices"], e["references"], e["materials"])
    else:
        sc = oracle.OracleScene(mrt.scene_path(cfg["scene"]), resolve_mtl(cfg))
    W, H = cfg["width"], cfg["height"]
    B = oracle.BVH
    if sc.n_triangles <= 64:
        rows = H                      # C2: the whole workload (all spp frames)
        rows1 = H
        f1 = min(2, frames)
    else:
        # a pilot band of 8 rows on all threads (after a first pass that
        # builds the BVH) gives the rate: one frame of a row band sized to
        # ~10 s on all threads, or whole frames when one takes less; ~10 s
        # on one thread
        pilot = np.zeros((H, W), np.uint8)
        pilot[(H - 8) // 2:(H - 8) // 2 + 8] = 1
        sc.render(W, H, cfg["L"], mrt.DEFAULT_SEED, 1, threads=threads, pixel_mask=pilot, flags=B)   # BVH build
        tp = time.perf_counter()
        sc.render(W, H, cfg["L"], mrt.DEFAULT_SEED, 1, threads=threads, pixel_mask=pilot, flags=B)
        per_row = max(1e-6, (time.perf_counter() - tp) / 8)
        rows = max(1, min(H, int(10.0 / per_row)))
        # a whole frame in < 10 s: several frames of the whole image, else one frame of the band
        frames = max(1, min(frames, int(10.0 / (per_row * H)))) if rows == H else 1
        rows1 = max(1, min(H, int(10.0 / (per_row * threads))))
        f1 = 1
    mask = np.zeros((H, W), np.uint8)
    y0 = (H - rows) // 2
    mask[y0:y0 + rows] = 1
    t0 = time.perf_counter()
    img, _ = sc.render(W, H, cfg["L"], mrt.DEFAULT_SEED, frames, threads=threads, pixel_mask=mask, flags=B)
    dt = time.perf_counter() - t0
    paths = W * rows * frames
    mask1 = np.zeros((H, W), np.uint8)
    y1 = (H - rows1) // 2
    mask1[y1:y1 + rows1] = 1
    t1 = time.perf_counter()
    sc.render(W, H, cfg["L"], mrt.DEFAULT_SEED, f1, threads=1, pixel_mask=mask1, flags=B)
    dt1 = time.perf_counter() - t1
    base = {"value": round(paths / dt / 1e6, 4), "unit": "Mpaths/s", "cores": threads, "kind": "port",
            "single_thread_value": round(W * rows1 * f1 / dt1 / 1e6, 4), "host_cpus": os.cpu_count(),
            "affinity_cpus": affinity_cpus(),
            "cores_policy": ("threads = the affinity mask capped by OMP_NUM_THREADS, the worker-pool size the GPU "
                             "pool sets for one GPU's CPU share of the shared host (its rule: size worker pools to "
                             "that share); the whole affinity mask is not used there"),
            "cpu_model": _cpu_model(),
            "sample": f"frames 0-{frames - 1}, rows {y0}-{y0 + rows - 1} of the workload ({W}x{rows} of {W}x{H}, "
                      f"L={cfg['L']}, {paths} paths), nearest hits through a binned-SAH BVH over "
                      f"{sc.n_triangles} triangles (same answers as brute force), "
                      f"{threads} std::threads over rows = the process's CPU share (affinity "
                      f"{len(os.sched_getaffinity(0))} of {os.cpu_count()} host CPUs, OMP_NUM_THREADS "
                      f"{os.environ.get('OMP_NUM_THREADS', '-')}), {dt:.2f} s wall; single thread: frames "
                      f"0-{f1 - 1} of rows {y1}-{y1 + rows1 - 1}, {dt1:.2f} s"}
    return base, img, mask, frames


def image_parity(gpu_img, ref_img, mask, build, frames, note):
    """Per-pixel relative L2 ||g - c|| / (||c|| + 1e-3) over RGB on the oracle's
    pixels (BASELINE.md image-match criterion), NaN-aware."""
    import numpy as np
    m = mask.astype(bool)
    g = gpu_img[m][:, :3].astype(np.float64)
    c = ref_img[m][:, :3].astype(np.float64)
    both_nan = np.isnan(g).any(-1) & np.isnan(c).any(-1)
    g, c = np.nan_to_num(g), np.nan_to_num(c)
    rel = np.where(both_nan, 0.0, np.sqrt(((g - c) ** 2).sum(-1)) / (np.sqrt((c ** 2).sum(-1)) + 1e-3))
    rmse = float(np.sqrt(((g - c) ** 2).mean()) / (np.sqrt((c ** 2).mean()) + 1e-12))
    same = float(((gpu_img[m][:, :3].view(np.uint32) == ref_img[m][:, :3].view(np.uint32)).all(-1) | both_nan).mean())
    return {"build": build, "vs": "CPU oracle (cpu_baseline leg's image)", "frames": frames, "pixels": int(m.sum()),
            "frac_rel_l2_le_1e-2": round(float((rel <= 1e-2).mean()), 6),
            "frac_rel_l2_le_1e-4": round(float((rel <= 1e-4).mean()), 6), "rel_rmse": float(f"{rmse:.3e}"),
            "bit_identical": round(same, 6), "max_rel_l2": float(f"{float(rel.max()):.3e}"),
            "gate": "fast: >= 0.99 of pixels within rel-L2 1e-2; precise: >= 0.999 within 1e-4 and rel-RMSE <= 1e-3",
            "pass": bool((rel <= 1e-2).mean() >= 0.99) if build == "fast" else
                    bool((rel <= 1e-4).mean() >= 0.999 and rmse <= 1e-3),
            "note": note}


def roofline(args, pmc_path, whole_frame, timed, launch_s, step_s, launches_per_step):
    """The hot kernel against its physical roofs, from the PMC passes of the
    same command (tools/profile.sh -> tools/prof_summary.py ->
    profiles/pmc_<config>.json; rocprofv3 --pmc has to wrap the process, so
    the counts come from that file, recorded with the md5 of the libmrt.so
    it measured) divided by this run's HIP-event launch time:
      hbm  — (2 x FETCH_SIZE + WRITE_SIZE) bytes per launch (MI355X_MICROARCH.md
             gfx950 correction) / launch time, against 8 TB/s;
      valu — SQ_INSTS_VALU x 64 lane-slots per launch / launch time, against
             1024 SIMDs x 32 lanes/cycle x 2.4 GHz (a wave64 VALU instruction
             holds its SIMD's issue for 2 cycles whatever its exec mask).
    bound = the roof with the larger fraction (the counter-measured limiter).
    Three clocks for the same per-launch counts: `frac` (the headline) divides
    by the wall-clock step time per launch (ms_per_step x steps / launches:
    includes the accumulate pass and launch gaps, never favourable);
    `frac_vs_launch` by this run's per-launch kernel time (HIP events, or the
    device span with launches on two streams); `frac_vs_profile` by the
    rocprofv3 trace's average duration of the same kernel (profiles/, one
    render stream).  valu_useful_* = the VALU fraction x valu_lane_util: the
    share of the issue roof doing work in active lanes."""
    import mrt
    out = {"bound": "unmeasured", "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None}
    if not (os.path.exists(pmc_path) and not args.precise and (args.pmc or whole_frame) and timed):
        out["note"] = ("no PMC passes for this command in profiles/ (they measure the whole frame of the fast "
                       "build on one GPU)")
        return out
    with open(pmc_path) as f:
        pmc = json.load(f)
    traffic = pmc.get("hbm_bytes_per_launch")
    valu_insts = (pmc.get("sq") or {}).get("SQ_INSTS_VALU")
    lane_util = pmc.get("valu_lane_util")
    step_launch_s = step_s / max(1e-9, launches_per_step)     # wall-clock step time per launch
    prof_s = (pmc.get("avg_launch_ns_rocprof_timed") or pmc.get("avg_launch_ns_rocprof") or 0) * 1e-9
    period_s = (pmc.get("period_ns_rocprof_2streams") or 0) * 1e-9
    roofs = {}

    def fracs(per_launch, peak):
        f = {"frac": round(per_launch / step_launch_s / peak, 4),
             "frac_vs_launch": round(per_launch / launch_s / peak, 4)}
        if prof_s:
            f["frac_vs_profile"] = round(per_launch / prof_s / peak, 4)
        if period_s:
            f["frac_vs_profile_period"] = round(per_launch / period_s / peak, 4)
        return f

    if traffic:
        gbs = traffic / step_launch_s / 1e9
        roofs["hbm"] = {"achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        **fracs(traffic / 1e9, HBM_PEAK_GBS), "bytes_per_launch": traffic}
    if valu_insts:
        t = valu_insts * 64 / step_launch_s / 1e12
        v = {"achieved": round(t, 2), "peak": round(VALU_PEAK_TLANE, 2), "unit": "T VALU lane-slots/s",
             **fracs(valu_insts * 64 / 1e12, VALU_PEAK_TLANE), "wave_instructions_per_launch": valu_insts}
        if lane_util:
            for k in ("frac", "frac_vs_launch", "frac_vs_profile", "frac_vs_profile_period"):
                if k in v:
                    v["valu_useful_" + k] = round(v[k] * lane_util, 4)
        roofs["valu-issue"] = v
    if not roofs:
        out["note"] = f"{os.path.basename(pmc_path)} holds no counts"
        return out
    bound = max(roofs, key=lambda k: roofs[k]["frac"])
    out.update({k: roofs[bound].get(k) for k in ("achieved", "peak", "unit", "frac", "frac_vs_launch",
                                                  "frac_vs_profile")})
    if "valu-issue" in roofs:
        out["valu_useful_frac"] = roofs["valu-issue"].get("valu_useful_frac")
    out.update({"bound": bound, "traffic": traffic, "roofs": roofs,
                "clocks": {"frac": f"wall-clock step time per launch {step_launch_s * 1e3:.4f} ms",
                           "frac_vs_launch": f"this run's per-launch kernel time {launch_s * 1e3:.4f} ms",
                           "frac_vs_profile": (f"rocprofv3 trace average {prof_s * 1e3:.4f} ms (one render "
                                               f"stream, timed launches)" if prof_s else None),
                           "frac_vs_profile_period": (f"rocprofv3 trace period {period_s * 1e3:.4f} ms per launch "
                                                      f"(two render streams)" if period_s else None)},
                "wait_any_frac": pmc.get("wait_any_frac"),
                "valu_lane_util": lane_util,
                "pmc_clock_ghz": pmc.get("clock_ghz"),
                "rocprof_avg_launch_ms": round(prof_s * 1e3, 4) if prof_s else None,
                "rocprof_timed_launches": pmc.get("timed_launches_rocprof"),
                "rocprof_period_ms_2streams": round(period_s * 1e3, 4) if period_s else None,
                "source": f"profiles/{os.path.basename(pmc_path)} (tag {pmc.get('tag')}, commit "
                          f"{pmc.get('commit', 'unrecorded')}, lib md5 {pmc.get('lib_md5')})",
                "same_library": (pmc.get("lib_md5") == lib_md5(mrt.LIB_PATH)) if pmc.get("lib_md5") else None})
    return out


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, img):
    """--dump-outputs: the timed path's result, the [H, W, 4] float32 image a
    caller reads back after the last timed step, as <out_dir>/image.npy.  An
    image above 64 MB (C5's 4K frame) is written as a fixed sample of its
    pixels, [n, 4] in ascending pixel order (row-major index y * W + x drawn
    with seed 0: the same pixels in every run of the same size)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    img = np.ascontiguousarray(img, np.float32)
    if img.nbytes > DUMP_MAX_BYTES:
        px = img.reshape(-1, img.shape[-1])
        n = DUMP_MAX_BYTES // (px.shape[1] * 4)
        idx = np.sort(np.random.default_rng(0).choice(px.shape[0], size=n, replace=False))
        img = np.ascontiguousarray(px[idx])
    np.save(os.path.join(out_dir, "image.npy"), img)


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.sweep_gpus):
        sys.exit(launch(args))   # N ranks started here, before any HIP call
    cfg = CONFIGS[args.config]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    shard_count = world
    if args.shard_of:
        if world > 1:
            raise SystemExit("--shard-of is a single-process diagnostic")
        shard_count = args.shard_of
    dist = None
    if world > 1:
        # imported before libmrt is loaded: torch's bundled HIP runtime and
        # RCCL carry the same sonames as ROCm's, so libmrt binds to the copies
        # already in the process (one runtime); torch itself never touches the GPU
        import torch
        import torch.distributed as dist   # CPU control plane (gloo) only
    import mrt
    ndev = mrt.device_count()
    if ndev == 0:
        raise SystemExit("no HIP device visible to libmrt")
    device = local_rank % ndev   # == local_rank on a full node
    if world > 1:
        dist.init_process_group("gloo")
    if args.max_path_length:
        cfg = dict(cfg, L=args.max_path_length, workload=cfg["workload"] + f" (L={args.max_path_length} override)")
    W, H, spp, L = cfg["width"], cfg["height"], cfg["spp"], cfg["L"]
    scene = mrt.Scene(cfg["scene"], resolve_mtl(cfg), procedural_triangles=cfg["procedural"], device=device,
                      bvh_builder={"sah": mrt.BVH_HOST_SAH, "lbvh": mrt.BVH_DEVICE_LBVH,
                                   "ploc": mrt.BVH_DEVICE_PLOC}[args.bvh])
    r = mrt.Renderer(scene, W, H, L, precise=args.precise, profile=not args.no_kernel_timing,
                     shard_rank=(args.shard_rank if args.shard_of else rank), shard_count=shard_count)
    per_frame = cfg.get("cadence") == "frame"
    if not per_frame:
        r.prepare(spp)
    prep = r.stats()   # noise chunk of the step's spp frames, generated + uploaded before the timed region

    # multi-GPU exchange: every rank's owned 64x64 tiles go
    # to rank 0 through libmrt's RCCL communicator (include/mrt.h
    # mrt_renderer_exchange), enqueued on the renderer's stream behind the
    # draw.  Default: gather of the densely packed owned tiles (1/N of the
    # image per rank), MRT_EXCHANGE_OVERLAP — the gather of step k runs on the
    # communicator's stream while step k+1 renders, and rank 0 unpacks it
    # (non-owned tiles only) at the next exchange; the packed tiles are
    # double-buffered and libmrt orders buffer reuse with events.  The last
    # step's exchange is flushed inside the timed region.
    comm = None
    mode = 0
    if world > 1 and args.exchange_backend == "rccl":
        uid = [mrt.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        comm = mrt.Comm(uid[0], world, rank, device)
        mode = (mrt.EXCHANGE_REDUCE if args.exchange == "reduce" else
                mrt.EXCHANGE_GATHER | (0 if args.no_overlap else mrt.EXCHANGE_OVERLAP))
    host_slab = mrt.tiles_packed_floats(W, H, 0, world) if world > 1 else 0

    def host_exchange():
        """Rehearsal transport (ranks may share a GPU): packed tiles to host,
        one gloo gather to rank 0, which writes them into its image."""
        mine = r.tiles_read(rank, world)
        buf = torch.zeros(host_slab, dtype=torch.float32)
        buf[:mine.size] = torch.from_numpy(mine)
        lst = [torch.zeros(host_slab, dtype=torch.float32) for _ in range(world)] if rank == 0 else None
        dist.gather(buf, lst, dst=0)
        if rank == 0:
            for k in range(1, world):
                r.tiles_write(k, lst[k].numpy()[:mrt.tiles_packed_floats(W, H, k, world)])

    def step():
        if per_frame:   # drawInMTKView: x spp, the image keeps accumulating
            for _ in range(spp):
                r.draw_frame()
            return
        r.reset()
        r.draw(spp)
        if world == 1:
            return
        if comm is not None:
            r.exchange(comm, mode)
        else:
            host_exchange()

    def finish():
        r.exchange_flush()
        r.sync()

    for _ in range(args.warmup):
        step()
    finish()
    base = r.stats()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    finish()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    st = r.stats()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, r.read_image())
    sustained = None
    if args.full and world == 1 and args.sustain > 0 and not per_frame:
        # a longer window of the same steps (~seconds, visible to an outside
        # utilisation sampler); the headline value stays the K timed steps
        n_s, t_s = 0, time.perf_counter()
        t_report = t_s
        while True:
            # no stream drain inside the window (a sync every few steps costs
            # the launches' overlap, ~1 % on C2): the host runs at most the
            # in-flight bound (3 draws) ahead, and the window ends with a sync
            step()
            n_s += 1
            now = time.perf_counter()
            if now - t_s >= args.sustain:
                break
            if now - t_report >= 30.0:   # progress for long windows (stderr)
                t_report = now
                print(f"sustain: {n_s} steps in {now - t_s:.1f} s", file=sys.stderr, flush=True)
        r.sync()
        dt_s = time.perf_counter() - t_s
        sustained = {"steps": n_s, "seconds": round(dt_s, 3),
                     "value": round((st["paths"] - base["paths"]) / max(1, args.steps) * n_s / dt_s / 1e6, 3),
                     "ms_per_step": round(dt_s / n_s * 1e3, 3),
                     "note": "the same step repeated for --sustain seconds after the timed region (reported "
                             "beside the line; value is the K timed steps)"}
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        tot = torch.tensor([st["paths"] - base["paths"]], dtype=torch.float64)
        dist.all_reduce(tot)
        assert int(tot.item()) == W * H * spp * args.steps, "ranks did not cover the frame"
    total_paths = W * H * spp * args.steps
    if args.shard_of:
        total_paths = st["paths"] - base["paths"]   # this GPU's share only
    ms_per_step = elapsed / args.steps * 1e3
    value = total_paths / elapsed / 1e6

    # Roofline of the dominant kernel (stream_kernel on C1/C2, path_kernel on
    # C3-C5: one launch per frame batch), its launch time measured live with
    # HIP events on the render stream around each batch's launch.  A tile
    # share renders batches on two streams (the next launch starts while one
    # drains), where events would also time the wait for CUs: there the
    # launch time is the device-measured span (earliest block start to latest
    # wave end, the chip's wall clock), which libmrt records for every batch.
    A = st["active_ray_bounces"] - base["active_ray_bounces"]
    P = st["paths"] - base["paths"]
    launches = st["kernel_launches"] - base["kernel_launches"]
    timed = st["timed_launches"] - base["timed_launches"]
    kms = st["kernel_ms"] - base["kernel_ms"]
    spans = st["spans"] - base["spans"]
    avg_span_ms = (st["span_ms"] - base["span_ms"]) / spans if spans else None
    bytes_alg = B_PATH * P + B_BOUNCE * A
    avg_launch_ms = kms / max(1, timed)
    launch_timing = "hip-events on the render stream"
    if st["inflight"] > 1 and spans and spans == launches:
        # a launch queued behind the previous one starts a few blocks early
        # and the rest once CUs free up, so its span can exceed its share of
        # the step: never more than the step's time per launch
        per_launch_ms = ms_per_step * args.steps / max(1, launches)
        avg_launch_ms, timed = min(avg_span_ms, per_launch_ms), spans
        launch_timing = ("device spans (launches on 2 streams overlap)" if avg_span_ms <= per_launch_ms
                         else "step time per launch (device spans of overlapped launches exceed it)")
    launch_s = avg_launch_ms * 1e-3
    launches_per_step = launches / max(1, args.steps)
    roof = roofline(args, pmc_path=args.pmc or os.path.join(ROOT, "profiles", f"pmc_{args.config}.json"),
                    whole_frame=shard_count == 1 and not args.max_path_length, timed=timed, launch_s=launch_s,
                    step_s=ms_per_step * 1e-3, launches_per_step=launches_per_step)
    # the reference's wavefront data contract (112 B per path +
    # 312 B per active ray-bounce) per launch / launch time: an EQUIVALENT
    # bandwidth — the bytes the reference's 2 + 4L passes would move, not
    # bytes this fused kernel moves (it keeps hits and shadow rays in
    # registers), so it can exceed the HBM peak and is not the roofline
    alg = (bytes_alg / max(1, launches)) / launch_s / 1e9 if timed else 0.0
    roof.update({
        "alg_equiv_gbs": round(alg, 1), "alg_equiv_frac": round(alg / HBM_PEAK_GBS, 4),
        "alg_equiv_note": "SURVEY 8(d) algorithmic bytes (the reference's 2+4L-pass AoS traffic) per launch / "
                          "launch time: the bytes the reference's wavefront would move, not this kernel's",
        "kernel": {1: "path_kernel (all bounces per launch)",
                   2: "stream_kernel (wave-local streaming wavefront: all bounces per launch)"}.get(
                       st["kernel"], "bounce_kernel (one launch per bounce)"),
        "launches": launches, "timed_launches": timed, "avg_launch_ms": round(avg_launch_ms, 4),
        "launch_timing": launch_timing,
        "avg_span_ms": None if avg_span_ms is None else round(avg_span_ms, 4),
        "alg_bytes_per_launch": int(bytes_alg / max(1, launches)),
        "active_ray_bounces_per_step": int(A / max(1, args.steps))})

    # the noise schedule's host cost: the reference regenerates
    # one 64x64 float4 table per frame on one CPU thread before the frame's
    # commit (renderer/Renderer.mm:486-496); libmrt generates the step's
    # window ahead of the timed region (mrt_renderer_prepare, host threads +
    # one upload).  Both per frame: a progressive render past the window pays
    # the latter inside draw.
    noise = {"noise_ms_per_frame": None,
             "prepare_ms_per_frame": round(prep["noise_ms"] / max(1, prep["noise_tables"]), 4),
             "prepare_tables": int(prep["noise_tables"]),
             "prepare_note": "mrt_renderer_prepare: the window's tables on the library's host threads + one "
                             "upload, per table"}
    if args.full:
        mrt.noise_table(mrt.DEFAULT_SEED, 0)   # first call imports numpy
        t_n = time.perf_counter()
        for f in range(32):
            mrt.noise_table(mrt.DEFAULT_SEED, f)
        noise_1t_ms = (time.perf_counter() - t_n) * 1e3 / 32
        noise.update({"noise_ms_per_frame": round(noise_1t_ms, 4),
                      "noise_ms_per_frame_note": "one table generated on one host thread (mrt_noise_table), the "
                                                 "reference's per-frame CPU cost model; not in the timed steps"})
    if per_frame:
        noise.update({"timed_tables": int(st["noise_tables"] - base["noise_tables"]),
                      "timed_gen_ms": round(st["noise_ms"] - base["noise_ms"], 3),
                      "timed_noise_waits": int(st["noise_waits"] - base["noise_waits"]),
                      "timed_prefetched_chunks": int(st["noise_prefetched"] - base["noise_prefetched"]),
                      "timed_note": "tables generated inside the timed steps on the noise worker thread "
                                    "(overlapped with rendering); waits = draws that waited for generation"})

    result = {
        "metric": METRIC,
        "value": round(value, 3),
        "unit": "Mpaths/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": f"reference scene renderer/Media/{cfg['scene']}.obj" +
                (f" + seeded procedural mesh ({cfg['procedural']} tris)" if cfg["procedural"] else "") +
                ", deterministic noise seed",
        "config": {"workload": cfg["workload"], "width": W, "height": H, "spp": spp, "max_path_length": L,
                   # MAX_PATH_LENGTH as renderer/Renderer.mm:517 loops it: L ray segments
                   # per path = the primary ray + (L - 1) bounces
                   "path_segments": f"primary ray + {L - 1} bounces",
                   "scene": cfg["scene"], "parallelism": (f"tile shard {args.shard_rank} of {shard_count} (one GPU's share)" if args.shard_of else
                                   f"tiles64x{world}" + ((f" + rccl {args.exchange}" + ("" if args.no_overlap or args.exchange == "reduce" else " (overlapped)")
                                                          if args.exchange_backend == "rccl" else " + host/gloo gather") if world > 1 else "")),
                   "build": "precise" if args.precise else "fast",
                   "bvh": {"builder": {"sah": "host-sah", "lbvh": "device-lbvh", "ploc": "device-ploc"}[args.bvh],
                           "build_ms": round(scene.info["build_ms"], 2), "nodes": scene.info["bvh_nodes"],
                           "max_stack": scene.info["bvh_max_stack"]}},
        "roofline": roof,
        "cpu_baseline": None,
        "noise_ms_per_frame": noise["noise_ms_per_frame"],
        "noise": noise,
    }
    if sustained:
        result["sustained"] = sustained
    if per_frame:
        result["cadence"] = {
            "draw_calls": int(st["draws"] - base["draws"]),
            "draws_overlapped": int(st["draws_overlapped"] - base["draws_overlapped"]),
            "inflight_waits": int(st["inflight_waits"] - base["inflight_waits"]),
            "ms_per_draw": round(elapsed * 1e3 / max(1, st["draws"] - base["draws"]), 4),
            "note": "draws_overlapped: calls enqueued while the previous draw still ran on the GPU; "
                    "inflight_waits: calls that waited for the draw 3 back (MaxBuffersInFlight, "
                    "renderer/Renderer.mm:16,593-600)"}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.shard_of:
        base_cpu, ref_img, mask, frames = cpu_baseline(cfg, args.cpu_frames or spp)
        result["cpu_baseline"] = base_cpu
        # image match vs the reference restatement (north_star): the timed
        # render itself when the oracle ran the whole workload (C2: all spp
        # frames, every pixel), else a render of the sampled frames; and the
        # same frames through the parity (precise) build
        par = []
        for precise in (args.precise, True) if not args.precise else (True,):
            if not precise and frames == spp and not per_frame:
                gimg = r.read_image()
                note = "the timed steps' image (last step: reset + all spp frames)"
            else:
                r1 = mrt.Renderer(scene, W, H, L, precise=precise)
                if per_frame:
                    for _ in range(frames):
                        r1.draw_frame()
                else:
                    r1.draw(frames)
                gimg = r1.read_image()
                r1.close()
                note = f"a separate render of frames 0-{frames - 1}" + (
                    " (one mrt_renderer_draw call per frame)" if per_frame else "")
            par.append(image_parity(gimg, ref_img, mask, "precise" if precise else "fast", frames, note))
        result["parity"] = par[0]
        if len(par) > 1:
            result["parity_precise"] = par[1]
    if args.full and per_frame and rank == 0 and world == 1 and not args.no_image_check:
        # the timed progressive image == the same frames drawn in 64-frame
        # batches (draw_n), bitwise
        total = int(st["frame_index"])
        r1 = mrt.Renderer(scene, W, H, L, precise=args.precise)
        r1.draw(total)
        same = r1.read_image()[..., :3].tobytes() == r.read_image()[..., :3].tobytes()
        r1.close()
        result["image_check"] = (f"timed image (frames 0-{total - 1}, one draw call each) bitwise equal to "
                                 f"draw_n({total})" if same else "MISMATCH vs draw_n")
        assert same, "per-frame draws differ from the batched render"
    if world > 1 and args.check_image:
        if rank == 0:   # the exchanged image == one device rendering the whole frame, bitwise
            got = r.read_image()
            r1 = mrt.Renderer(scene, W, H, L, precise=args.precise)
            r1.draw(spp)
            ref = r1.read_image()
            r1.close()
            import numpy as np
            n_diff = int((got[..., :3] != ref[..., :3]).any(-1).sum())
            same = n_diff == 0
            result["image_check"] = ("bitwise equal to the 1-GPU render" if same else
                                     f"MISMATCH: {n_diff} of {W * H} pixels differ from the 1-GPU render")
            result["image_check_pixels_differing"] = n_diff
            if not same and args.check_image_tolerance:
                # opt-in gate (--check-image-tolerance): <= 1e-5 of the pixels,
                # each within rel-L2 1e-3.  The default is bitwise: the near-tie
                # order dependence of DESIGN §3.1 is fixed by the culling slack
                g, c = got[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
                rel = np.sqrt(((g - c) ** 2).sum(-1)) / (np.sqrt((c ** 2).sum(-1)) + 1e-3)
                same = n_diff <= 1e-5 * W * H and float(rel.max()) <= 1e-3
                result["image_check"] = (f"{n_diff} of {W * H} pixels differ from the 1-GPU render, max rel-L2 "
                                         f"{float(rel.max()):.2e} (within the --check-image-tolerance gate)"
                                         if same else result["image_check"])
            if not same:   # which tiles (and whose) differ
                import numpy as np
                diff = (got[..., :3] != ref[..., :3]).any(-1)
                ys, xs = np.nonzero(diff)
                tx = (W + 63) // 64
                owners = sorted({int((x // 64 + (y // 64) * tx) % world) for x, y in zip(xs[:100000], ys[:100000])})
                print(f"bench.py: image check: {int(diff.sum())} pixels differ; owners {owners}; first "
                      f"{list(zip(xs[:4].tolist(), ys[:4].tolist()))} got {got[ys[0], xs[0]].tolist()} "
                      f"ref {ref[ys[0], xs[0]].tolist()}", file=sys.stderr, flush=True)
            assert same, "exchanged image differs from the single-device render"
        dist.barrier()
    if rank == 0:
        print(json.dumps(result), flush=True)
    r.close()
    if comm is not None:
        comm.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
