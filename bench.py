#!/usr/bin/env python3
"""Benchmark: scan-to-map point-to-plane ICP (GN to convergence) on MI355X.

One *step* = one scan's IterativeClosestPointOptimizer::optimize (<= max_iterations GN iterations with PKO)
per GPU, against a frozen device-resident surfel map, scan points already resident in HBM.
Multi-GPU is scan-parallel (weak scaling): every rank owns its own map and scan stream; after each step the
ranks all-gather their 16-float pose/status records over RCCL (the only collective; no map sharding).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config kitti|mid360|patch1m] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...

Prints ONE JSON line on rank 0 (driver contract).  A plain run sets up, warms up, times the K steps and prints the
line; --dump-outputs DIR also writes what the last timed step returned as DIR/<name>.npy.  --full adds every other
measurement and check to the line (value spread, per-kernel times and rooflines, live PMC traffic, pipeline-off and
other-mode rates, PCIe-inclusive rate, multi-sequence and batched legs, the C5 leg, CPU baseline and parity).  The
CPU baseline is the oracle restatement of the reference ICP (single thread) timed on a bounded sample of the same
scans.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
MALL_BYTES = 256 << 20     # Infinity Cache (MALL) capacity
METRIC = "ICP GN-iterations/sec and scans/sec on KITTI-07 @ 1/2/4/8 GPU; % HBM BW"
ORDER = "azimuth"          # patch1m point order (--order)


_T_START = time.perf_counter()


def over_budget(args) -> bool:
    """--full: True once the process has run longer than --full-budget seconds; the batched sizes still to come and
    the C5 leg are then skipped (and named in the line), so that the run ends in bounded time on a slow host."""
    return time.perf_counter() - _T_START > args.full_budget


def log(*a):
    print(*a, file=sys.stderr, flush=True)


_JSON_OUT = None


def emit(result: dict):
    """Print the ONE JSON line on the original stdout.  Native libraries (gloo, RCCL, HIP) print to fd 1 too, so
    once the ranks are up fd 1 points at stderr and only this line reaches stdout."""
    out = _JSON_OUT or sys.stdout
    out.write(json.dumps(result) + "\n")
    out.flush()


def _claim_stdout():
    global _JSON_OUT
    if _JSON_OUT is None:
        sys.stdout.flush()
        _JSON_OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def dump_outputs(path: str, arrays: dict):
    """--dump-outputs: what the last timed step returned to its caller, one <name>.npy per array (float64 for
    double and integer fields, float32 otherwise), so that two builds can be compared output for output."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(path, name + ".npy"), a.astype(np.float32 if a.dtype == np.float32 else np.float64))


def icp_result_arrays(L, icp) -> dict:
    """lo_icp_result of the context's last enqueued scan (what a caller of lo_icp_optimize_async reads back): the
    pose, the status / iteration count / correspondence count / costs, and the per-iteration logs."""
    from lidar_odometry_amd._lib import LoIterLog, LoStats
    T = np.zeros(12, np.float32)
    logs = (LoIterLog * icp._cfg.max_iterations)()
    st = LoStats()
    rc = L.lo_icp_result(icp.ctx, T.ctypes.data_as(C.POINTER(C.c_float)), logs, C.byref(st))
    if rc < 0:
        raise RuntimeError(f"lo_icp_result rc={rc}: {L.lo_last_error(icp.ctx).decode()}")
    its = [logs[i] for i in range(min(st.iterations, len(logs)))]
    return {"pose": T.reshape(3, 4),
            "stats": np.array([st.status, st.iterations, st.n_corr, st.initial_cost, st.final_cost], np.float64),
            "iter_pose": np.array([x.pose[:] for x in its], np.float32).reshape(-1, 12),
            "iter_n_corr": np.array([x.n_corr for x in its], np.float64),
            "iter_scale": np.array([x.scale for x in its], np.float64),
            "iter_alpha": np.array([x.alpha for x in its], np.float64),
            "iter_cost": np.array([x.cost for x in its], np.float32),
            "iter_H": np.array([x.H[:] for x in its], np.float32).reshape(-1, 21),
            "iter_g": np.array([x.g[:] for x in its], np.float32).reshape(-1, 6),
            "iter_delta": np.array([x.delta[:] for x in its], np.float32).reshape(-1, 6)}


# --------------------------------------------------------------------------------------------------
# workloads (product-side data path only: synth + lo_voxelmap + lo_voxel_filter)
# --------------------------------------------------------------------------------------------------
def _raycast_device(rank: int):
    """Device for generating the synthetic scans (torch raycast on the rank's GPU; numpy on a CPU-only host)."""
    import torch
    if not torch.cuda.is_available():
        return None
    return f"cuda:{int(os.environ.get('LOCAL_RANK', rank)) % max(torch.cuda.device_count(), 1)}"


def build_kitti(rank: int, n_map: int = 660, name: str = "", city: bool = True):
    """KITTI-07-like workload: the surfel map after n_map frames of keyframing (a keyframe every
    2 frames ~ 1.2 m, kitti.yaml keyframe_distance 1.0; UpdateVoxelMap prunes to 1.2 x 100 m), then 20 scans from the
    last 40 frames between keyframes with perturbed initial poses.  city: the HDL-64-like scanner on a serpentine
    through a street grid (synth.KittiCitySequence), so the 120 m radius holds several streets and the map reaches
    ~10^4 L1 surfels; otherwise the single meandering street (KittiLikeSequence, the round-1 scene)."""
    from lidar_odometry_amd import synth
    from lidar_odometry_amd.voxelmap import VoxelMap, voxel_filter
    dev = _raycast_device(rank)
    seq = synth.KittiCitySequence(n_frames=n_map + 2) if city else synth.KittiLikeSequence(seed=7, n_frames=n_map + 2)
    vm = VoxelMap(0.5, 3, 0.1, True)
    kf = []
    for k in range(0, n_map + 1, 2):
        pts = voxel_filter(seq.scan(k, device=dev), 0.5, 8)     # FastVoxelFilter, point_stride 8, voxel 0.5
        T = seq.poses[k]
        w = synth.transform(T, pts)
        vm.update(w, T[:3, 3], 120.0, True)         # UpdateVoxelMap(.., 1.2 * max_range)
        kf.append((w, T[:3, 3].copy()))
    rng = np.random.default_rng(42 + rank)
    scans, inits, gts, frames = [], [], [], list(range(n_map - 39, n_map, 2))
    for f in frames:
        scans.append(voxel_filter(seq.scan(f, device=dev), 0.5, 8))
        inits.append(synth.perturb(seq.poses[f], rng, 0.05, 0.01))
        gts.append(seq.poses[f])
    return {"name": name or f"KITTI-07-like HDL-64 scan (stride 8, 0.5 m voxels) surfel ICP, config/kitti.yaml, city-grid "
                            f"map after {n_map} frames",
            "voxel": 0.5, "max_dist": 120.0, "vm": vm, "scans": scans, "inits": inits, "gts": gts, "keyframes": kf,
            "seq": seq, "frames": frames, "raycast_device": dev}


def build_kitti_small(rank: int):
    """Round-1 workload, kept as a labelled secondary line: the map after 42 frames (1.5k surfels)."""
    return build_kitti(rank, n_map=40, name="KITTI-07-like HDL-64 scan surfel ICP, small map (42 frames, round-1 line)",
                       city=False)


def build_mid360(rank: int):
    from lidar_odometry_amd import synth
    from lidar_odometry_amd.voxelmap import VoxelMap, voxel_filter
    sc = synth.mid360_scene()
    poses = [synth.se3(synth.rot_z(0.05 * k), [0.3 * k, 0.1 * k, 1.0]) for k in range(42)]
    vm = VoxelMap(0.4, 3, 0.1, True)
    kf = []
    for k in range(0, 41, 2):
        p = voxel_filter(synth.mid360_like_scan(sc, poses[k], k), 0.4, 4)
        w = synth.transform(poses[k], p)
        vm.update(w, poses[k][:3, 3], 48.0, True)
        kf.append((w, poses[k][:3, 3].copy()))
    rng = np.random.default_rng(142 + rank)
    scans, inits, gts = [], [], []
    for f in range(1, 40, 2):
        scans.append(voxel_filter(synth.mid360_like_scan(sc, poses[f], f), 0.4, 4))
        inits.append(synth.perturb(poses[f], rng, 0.05, 0.01))
        gts.append(poses[f])
    return {"name": "MID360-like rosette scan (stride 4, 0.4 m voxels) surfel ICP, config/mid360.yaml (surfel forced)",
            "voxel": 0.4, "max_dist": 48.0, "vm": vm, "scans": scans, "inits": inits, "gts": gts, "keyframes": kf}


def build_patch1m(rank: int):
    from lidar_odometry_amd import synth
    from lidar_odometry_amd.voxelmap import VoxelMap
    sc = synth.patch_scene(1000, 1000 + rank)
    vm = VoxelMap(0.5, 3, 0.1, True)
    mp = synth.sample_patches(sc, 1_500_000, 1007 + rank, sigma=0.01, outlier_frac=0.0)
    vm.update(mp, np.zeros(3), 1e4, True)
    rng = np.random.default_rng(1000 + rank)
    scans, inits, gts = [], [], []
    for f in range(4):
        T = synth.se3(synth.rot_z(0.3 + 0.1 * f), [1.0 + f, -2.0, 0.5])
        world = synth.sample_patches(sc, 1_000_000, 1011 + 10 * f + rank)
        local = synth.transform(np.linalg.inv(T), world)
        # acquisition order of a spinning sensor (azimuth); --order random keeps the generator's permutation
        scans.append(local if ORDER == "random" else synth.azimuth_order(local))
        inits.append(synth.perturb(T, rng, 0.05, 0.01))
        gts.append(T)
    return {"name": f"synthetic 1M-pt scan, 1000 planar patches + 10% outliers, surfel ICP, {ORDER} point order",
            "voxel": 0.5, "max_dist": 1e4, "vm": vm, "scans": scans, "inits": inits, "gts": gts,
            "keyframes": [(mp, np.zeros(3))]}


def build_kitti_raw(rank: int):
    """Raw HDL-64 scans: the step is Estimator::preprocess_frame (device FastVoxelFilter, stride 8, 0.5 m) + optimize."""
    wl = build_kitti(rank)
    wl["raw_scans"] = [wl["seq"].scan(f, device=wl["raycast_device"]) for f in wl["frames"]]
    wl["name"] = "KITTI-07-like raw HDL-64 scan -> device voxel filter (stride 8, 0.5 m) -> surfel ICP, config/kitti.yaml"
    wl["raw"] = True
    return wl


def build_kitti_kdtree(rank: int):
    wl = build_kitti(rank)
    wl["name"] = "KITTI-07-like HDL-64 scan, KDTree correspondence variant (5-NN plane fit), config/kitti.yaml"
    wl["kdtree"] = True
    return wl


WORKLOADS = {"kitti": build_kitti, "kitti_small": build_kitti_small, "kitti_raw": build_kitti_raw, "kitti_kdtree": build_kitti_kdtree, "mid360": build_mid360,
             "patch1m": build_patch1m}


def pose12(T):
    return np.ascontiguousarray(np.asarray(T, np.float64)[:3, :].astype(np.float32).reshape(12))


# --------------------------------------------------------------------------------------------------
# CPU baseline: oracle restatement of the reference ICP, 1 thread, bounded sample
# --------------------------------------------------------------------------------------------------
def _rot_diff(A12, B12) -> float:
    """Rotation difference (rad) of two row-major 3x4 poses: ||Ra - Rb||_F / sqrt(2) ~ the angle."""
    a = np.asarray(A12, np.float64).reshape(3, 4)[:, :3]
    b = np.asarray(B12, np.float64).reshape(3, 4)[:, :3]
    return float(np.linalg.norm(a - b) / np.sqrt(2.0))


def parity_vs_oracle(gpu, cpu) -> dict:
    """The GPU's optimize() results against the oracle's on the same scans (north_star: 1e-4 m / 1e-4 rad per
    iteration on identical inputs).  gpu / cpu: per scan {"ok", "T" (12), "logs" (per-iteration dicts)}."""
    dt = dr = dt_it = dr_it = 0.0
    same_iters = same_alpha0 = same_alpha_all = same_ok = 0
    for g, c in zip(gpu, cpu):
        same_ok += int(g["ok"] == c["ok"])
        dt = max(dt, float(np.abs(np.asarray(g["T"], np.float64).reshape(3, 4)[:, 3]
                                  - np.asarray(c["T"], np.float64).reshape(3, 4)[:, 3]).max()))
        dr = max(dr, _rot_diff(g["T"], c["T"]))
        same_iters += int(len(g["logs"]) == len(c["logs"]))
        if g["logs"] and c["logs"]:
            same_alpha0 += int(g["logs"][0]["alpha"] == c["logs"][0]["alpha"])
        same_alpha_all += int(len(g["logs"]) == len(c["logs"]) and
                              all(a["alpha"] == b["alpha"] for a, b in zip(g["logs"], c["logs"])))
        for a, b in zip(g["logs"], c["logs"]):
            dt_it = max(dt_it, float(np.abs(np.asarray(a["pose"], np.float64).reshape(3, 4)[:, 3]
                                            - np.asarray(b["pose"], np.float64).reshape(3, 4)[:, 3]).max()))
            dr_it = max(dr_it, _rot_diff(a["pose"], b["pose"]))
    n = len(gpu)
    return {"scans": n, "max_abs_dt_m": dt, "max_abs_dR_rad": dr, "per_iteration_max_dt_m": dt_it,
            "per_iteration_max_dR_rad": dr_it, "within_1e-4": bool(dt_it <= 1e-4 and dr_it <= 1e-4),
            "status_equal": same_ok, "iteration_count_equal": same_iters, "alpha_iter0_equal": same_alpha0,
            "alpha_every_iteration_equal": same_alpha_all}


def parity_bitwise(gpu, ref) -> int:
    """Scans whose every iteration's pose, alpha and n_corr, the final pose and the status equal the oracle's bits."""
    return sum(int(g["ok"] == c["ok"] and np.array_equal(np.asarray(g["T"], np.float32).view(np.uint32),
                                                        np.asarray(c["T"], np.float32).view(np.uint32))
                   and len(g["logs"]) == len(c["logs"])
                   and all(np.array_equal(np.asarray(a["pose"], np.float32).view(np.uint32),
                                          np.asarray(b["pose"], np.float32).view(np.uint32)) and
                           a["alpha"] == b["alpha"] and a["n_corr"] == b["n_corr"] for a, b in zip(g["logs"], c["logs"])))
               for g, c in zip(gpu, ref))


MODE_NOTE = {"exact": "lo_set_exact: the reference's fp32 operation order (sequential sums in correspondence order, "
                      "sorted-order iteration-0 scale, fp32 LDLT, JacobiSVD-projected SO3)",
             "fast": "lo_set_exact(ctx, 0): fp64 tree sums, Chan-merged iteration-0 scale, fp64 LDLT + polar SO3"}


def oracle_reference(wl):
    """The oracle's optimize() on every distinct scan of the workload (the parity reference)."""
    import oracle
    m = oracle.VoxelMap(wl["voxel"], 3, 0.1, True)
    for w, s in wl["keyframes"]:
        m.update(w, s, wl["max_dist"], True)
    ref = []
    for i, T in enumerate(wl["inits"]):
        pts_i = oracle.voxel_filter(wl["raw_scans"][i], 0.5, 8) if wl.get("raw") else wl["scans"][i]
        ok, To, _, logs = oracle.icp_optimize(m, pts_i, pose12(T), kdtree=wl.get("kdtree", False))
        ref.append({"ok": ok, "T": np.asarray(To if ok else pose12(T), np.float32), "logs": logs})
    return ref


def cpu_baseline(wl, budget_s: float, gpu_by_mode=None, value_mode="exact"):
    """The oracle port timed on this host (1 thread, bounded sample); its first pass over the distinct scans is also
    the parity reference for the GPU results of the same scans, per arithmetic mode (gpu_by_mode: {mode: results});
    `parity` is the mode reported as value, `parity_other` the other one."""
    import oracle
    m = oracle.VoxelMap(wl["voxel"], 3, 0.1, True)
    for w, s in wl["keyframes"]:
        m.update(w, s, wl["max_dist"], True)
    scans, inits = wl["scans"], [pose12(T) for T in wl["inits"]]
    n_scans = n_iters = 0
    ref = []
    t0 = time.perf_counter()
    while True:
        i = n_scans % len(scans)
        pts_i = oracle.voxel_filter(wl["raw_scans"][i], 0.5, 8) if wl.get("raw") else scans[i]
        ok, To, it, logs = oracle.icp_optimize(m, pts_i, inits[i], kdtree=wl.get("kdtree", False))
        if n_scans < len(scans):
            ref.append({"ok": ok, "T": np.asarray(To if ok else inits[i], np.float32), "logs": logs})
        n_scans += 1
        n_iters += it
        el = time.perf_counter() - t0
        if el >= budget_s and n_scans >= len(scans):
            break
    out = {"value": n_scans / el, "unit": "scans/s", "cores": 1, "kind": "port",
           "gn_iters_per_sec": n_iters / el,
           "sample": f"{n_scans} optimize() calls over {len(scans)} distinct scans in {el:.1f} s "
                     f"(oracle/liblo_oracle.so, single thread, g++ -O3, same synthetic inputs)"}
    for mode, gpu in (gpu_by_mode or {}).items():
        if gpu is None:
            continue
        p = parity_vs_oracle(gpu, ref)
        p["bitwise_equal"] = parity_bitwise(gpu, ref)
        p["mode"] = mode
        p["mode_note"] = MODE_NOTE[mode]
        out["parity" if mode == value_mode else "parity_other"] = p
    return out


def cpu_baseline_replicas(wl, budget_s: float, threads: int):
    """The fair CPU comparator for the batched (multi-sequence) number: `threads` independent
    replicas of the single-thread oracle ICP, one per core, each with its own map copy and scan stream.  The oracle
    is a C library called through ctypes (GIL released during the call), so Python threads run it in parallel."""
    import concurrent.futures as cf

    import oracle
    scans, inits = wl["scans"], [pose12(T) for T in wl["inits"]]

    def replica(r):
        m = oracle.VoxelMap(wl["voxel"], 3, 0.1, True)
        for w, s in wl["keyframes"]:
            m.update(w, s, wl["max_dist"], True)
        n = 0
        t0 = time.perf_counter()
        while True:
            i = (n + 7 * r) % len(scans)
            oracle.icp_optimize(m, scans[i], inits[i])
            n += 1
            el = time.perf_counter() - t0
            if el >= budget_s:
                return n, el

    with cf.ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(replica, range(threads)))
    n = sum(r[0] for r in res)
    el = max(r[1] for r in res)
    return {"value": n / el, "unit": "scans/s", "cores": threads, "kind": "port",
            "sample": f"{threads} concurrent single-thread oracle replicas (own map each), {n} optimize() calls in "
                      f"{el:.1f} s on the GPU box's host cores"}


def read_pmc_traffic(workload_key: str):
    """HBM bytes per k_correspond launch from a committed rocprofv3 PMC summary (profiles/), if present."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(p) as f:
            d = json.load(f)
        e = d.get(workload_key)
        return None if e is None else float(e["hbm_bytes_per_launch"])
    except Exception:
        return None


def pmc_child(path: str):
    """--pmc-child: the isolated k_correspond launches of a case the parent bench wrote (scan, pose, scale/alpha,
    surfel map), nothing else -- the program rocprofv3 --pmc runs for live_pmc."""
    import torch
    from lidar_odometry_amd import lib
    from lidar_odometry_amd.icp import IterativeClosestPointOptimizer, MapGeometry
    z = np.load(path)
    if "batch" in z:                       # the batched launch: B contexts (own map copy each), private scan copies
        from lidar_odometry_amd import BatchOptimizer
        B, nd = int(z["batch"]), int(z["n_scans"])
        scans = [np.ascontiguousarray(z[f"scan_{i}"], np.float32) for i in range(nd)]
        inits = np.ascontiguousarray(z["inits"], np.float32).reshape(nd, 12)
        mp = max(len(x) for x in scans)
        ctxs = []
        for _ in range(B):
            o = IterativeClosestPointOptimizer(geometry=MapGeometry(voxel_size=float(z["voxel"])), max_points=mp)
            o.set_surfels(z["keys"], z["normals"], z["centroids"])
            ctxs.append(o)
        bo = BatchOptimizer(ctxs)
        sel = [j % nd for j in range(B)]
        job = [torch.from_numpy(scans[i]).cuda() for i in sel]
        c_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in job])
        c_cnts = (C.c_size_t * B)(*[t.shape[0] for t in job])
        c_T = np.ascontiguousarray(np.stack([inits[i] for i in sel]))
        from lidar_odometry_amd._lib import LoBatchRec
        recs = (LoBatchRec * B)()
        ms = C.c_double(0.0)
        L = lib()
        rc = L.lo_batch_optimize_async(bo._b, c_ptrs, c_cnts, c_T.ctypes.data_as(C.POINTER(C.c_float)))
        rc |= L.lo_batch_result(bo._b, recs, C.byref(ms))
        cms = C.c_float(0.0)
        rc |= L.lo_batch_bench_correspond(bo._b, int(z["reps"]), C.byref(cms))
        torch.cuda.synchronize()
        bo.close()
        for o in ctxs:
            o.close()
        sys.exit(0 if rc == 0 else 1)
    pts = np.ascontiguousarray(z["pts"], np.float32)
    icp = IterativeClosestPointOptimizer(geometry=MapGeometry(voxel_size=float(z["voxel"])), max_points=len(pts))
    icp.set_surfels(z["keys"], z["normals"], z["centroids"])
    d = torch.from_numpy(pts).cuda()
    T = np.ascontiguousarray(z["T"], np.float32)
    ms = C.c_float(0.0)
    rc = lib().lo_bench_kernel(icp.ctx, C.c_void_p(d.data_ptr()), len(pts), T.ctypes.data_as(C.POINTER(C.c_float)),
                               C.c_double(float(z["scale"])), C.c_double(float(z["alpha"])), 0, int(z["reps"]),
                               C.byref(ms))
    torch.cuda.synchronize()
    icp.close()
    sys.exit(0 if rc == 0 else 1)


def live_pmc(case: dict, reps: int = 200, kernel: str = "k_correspond"):
    """HBM traffic of one k_correspond launch, measured in this run: two rocprofv3 passes (--pmc FETCH_SIZE, then
    --pmc WRITE_SIZE, each counter in a run of its own) over `reps` isolated launches of the bench's largest scan,
    in child processes (this process has initialised the GPU).  MI355X_MICROARCH.md §HBM: the counters are KiB;
    FETCH_SIZE counts half of a wide coalesced stream's bytes on gfx950, so the read side is taken x2 (the raw
    values are kept).  Returns None when rocprofv3 is absent or a pass fails."""
    import shutil
    import subprocess
    import tempfile
    if not shutil.which("rocprofv3"):
        return None
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from pmc_summary import per_launch
    out = {}
    with tempfile.TemporaryDirectory(prefix="lo_pmc_") as tmp:
        np.savez(os.path.join(tmp, "case.npz"), reps=reps, **case)
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = ["timeout", "-s", "KILL", "240", "rocprofv3", "--pmc", counter, "--kernel-trace",
                   "--kernel-include-regex", kernel, "-d", d, "-o", "run", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child", os.path.join(tmp, "case.npz")]
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, cwd=ROOT)
            if r.returncode != 0:
                log(f"live PMC pass {counter} failed (rc {r.returncode}): {r.stderr.decode(errors='replace')[-400:]}")
                return None
            try:
                iso, n_iso, _, _ = per_launch(d, counter, kernel, min_run=20)
            except SystemExit as e:
                log(f"live PMC pass {counter}: {e}")
                return None
            out[counter] = (iso, n_iso)
    fetch_kib, nf = out["FETCH_SIZE"]
    write_kib, nw = out["WRITE_SIZE"]
    return {"hbm_bytes_per_launch": 2.0 * fetch_kib * 1024.0 + write_kib * 1024.0,
            "fetch_size_kib_raw": fetch_kib, "write_size_kib_raw": write_kib, "launches": [nf, nw],
            "correction": "FETCH_SIZE x2 (gfx950, MI355X_MICROARCH.md §HBM); memory-side counters, Infinity-Cache "
                          "hits included"}


def pko_roofline(em_live):
    """The dominant kernel's latency roofline (k_pko_t: a strictly sequential fp64 EM chain, neither HBM- nor
    MFMA-bound): cycles per EM iteration measured in this run (em_live: the lead PKO workgroup's s_memtime around its
    EM loop inside the bench's GN loop) against the issue floor of the loop's own instruction stream (the ISA count
    and measured instruction costs committed in profiles/pko_latency.json: scripts/pko_em_isa.py over the gfx950
    assembly, scripts/lat_bench.hip on the MI355X)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pko_latency.json")) as f:
            floor = json.load(f)
    except Exception:
        floor = {}
    achieved = em_live.get("cycles_per_em_iteration")
    peak = floor.get("peak")
    return {"kernel": "k_pko_t", "bound": "latency", "unit": "cycles per EM iteration",
            "achieved": achieved, "peak": peak, "frac": (peak / achieved) if (achieved and peak) else None,
            "measured_live": em_live,
            "floor_model": {k: floor.get(k) for k in ("floor_model", "isa_counts", "issue_cost_cycles", "isa_by")},
            "note": "lower is better: frac = issue floor / measured cycles; the EM must stay fp64 with the reference's "
                    "iteration count for alpha to stay identical"}


def c5_hbm_leg(local: int, dev, n_scans: int, pmc: bool = False, mode: str = "exact"):
    """C5's data at one GPU's scale (BASELINE.json configs[4]: synthetic 1M-point scans, 1000 planar patches + 10 %
    outliers): n_scans DISTINCT scans, each on its own context (its own slot / residual outputs and table copy),
    launched round-robin on one stream.  Between two launches of a scan the other n_scans - 1 move their own ~24 MB
    each, so the working set exceeds the 256 MB Infinity Cache and every correspondence launch reads its scan from
    HBM.  Reports k_correspond against the HBM roofline (isolated single launches with no set-up pass, and in-step:
    each scan's first correspondence launch inside its GN loop) and the 1M-point optimize rate."""
    import torch

    from lidar_odometry_amd import lib, synth
    from lidar_odometry_amd.icp import AdaptiveMEstimatorConfig, ICPConfig, IterativeClosestPointOptimizer, MapGeometry
    from lidar_odometry_amd.voxelmap import VoxelMap
    L = lib()
    t0 = time.perf_counter()
    sc = synth.patch_scene(1000, 1000)
    vm = VoxelMap(0.5, 3, 0.1, True)
    vm.update(synth.sample_patches(sc, 1_500_000, 1007, sigma=0.01, outlier_frac=0.0), np.zeros(3), 1e4, True)
    rng = np.random.default_rng(1000)
    stream = torch.cuda.Stream(dev)
    fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    ctxs, d_scans, scans, inits = [], [], [], []
    for f in range(n_scans):
        T = synth.se3(synth.rot_z(0.2 + 0.05 * f), [1.0 + 0.3 * f, -2.0, 0.5])
        pts = synth.azimuth_order(synth.transform(np.linalg.inv(T), synth.sample_patches(sc, 1_000_000, 2011 + f)))
        o = IterativeClosestPointOptimizer(ICPConfig(), AdaptiveMEstimatorConfig(), MapGeometry(voxel_size=0.5),
                                           device=local, max_points=len(pts))
        o.set_exact(mode == "exact")
        assert L.lo_map_set_from_voxelmap(o.ctx, vm.handle) == 0
        ctxs.append(o)
        scans.append(pts)
        inits.append(pose12(synth.perturb(T, rng, 0.05, 0.01)))
        d_scans.append(torch.from_numpy(pts).to(dev))
    log(f"[c5] {n_scans} distinct 1M-point scans built in {time.perf_counter() - t0:.1f} s, "
        f"{vm.surfel_count()} surfels")
    alg, it0, iters = [], [], []
    for o, p, Ti in zip(ctxs, scans, inits):
        o.optimize(None, p, Ti)
        st = o.get_last_stats()
        it0.append((float(st.iterations[0]["scale"]), float(st.iterations[0]["alpha"])))
        iters.append(st.num_iterations)
        nv, _, _ = o.find_correspondences(p, Ti)
        alg.append(len(p) * (12 + 8 + 4 + 8 + 0.125) + 24 * nv)
    for o in ctxs:
        L.lo_set_stream(o.ctx, C.c_void_p(stream.cuda_stream))
    # working set between two launches of one scan: every scan's points + its context's outputs + its table copy
    tab_bytes = 32 * 4 * vm.surfel_count()
    ws = sum(len(p) * (12 + 4 + 8) for p in scans) + n_scans * tab_bytes
    # isolated: one launch per call, no set-up pass, round-robin over the scans (each last touched n_scans - 1 ago)
    # timed two ways: the launch's own span (lo_bench_kernel 5: first block's start to last block's end, what a kernel
    # trace reports) and HIP events around the single launch (4: adds the dispatch latency, several us here)
    iso_us, iso_ev_us, iso_bytes = [], [], []
    for r in range(4):
        for kid in (5, 4):
            for i, o in enumerate(ctxs):
                ms = C.c_float(0.0)
                assert L.lo_bench_kernel(o.ctx, C.c_void_p(d_scans[i].data_ptr()), d_scans[i].shape[0], fptr(inits[i]),
                                         C.c_double(it0[i][0]), C.c_double(it0[i][1]), kid, 1, C.byref(ms)) == 0
                if r > 0 and ms.value > 0:
                    (iso_us if kid == 5 else iso_ev_us).append(ms.value * 1e3)
                    if kid == 5:
                        iso_bytes.append(alg[i])
    iso_t = float(np.mean(iso_us))
    iso_ach = float(np.mean(iso_bytes)) / (iso_t * 1e-6) / 1e9
    # primary (r06): back-to-back round-robin launches, HIP events around the whole sequence -- the per-launch device
    # time a kernel trace reproduces (its duration plus the dispatch gap); the span above leaves out the wave-launch ramp
    # and the end-of-kernel drain, single-launch events add the dispatch latency
    rr_rounds = 8
    arr_ctx = (C.c_void_p * n_scans)(*[o.ctx for o in ctxs])
    arr_pts = (C.c_void_p * n_scans)(*[d.data_ptr() for d in d_scans])
    arr_n = (C.c_size_t * n_scans)(*[d.shape[0] for d in d_scans])
    T_all = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float32).reshape(12) for t in inits]))
    rr_us = []
    for r in range(3):
        ms = C.c_float(0.0)
        assert L.lo_bench_correspond_rr(arr_ctx, arr_pts, arr_n, fptr(T_all), n_scans, rr_rounds, C.byref(ms)) == 0
        if r > 0:
            rr_us.append(ms.value * 1e3)
    rr_t = float(np.median(rr_us))
    rr_ach = float(np.mean(alg)) / (rr_t * 1e-6) / 1e9

    def enqueue_round():
        for i, o in enumerate(ctxs):
            assert L.lo_icp_optimize_async(o.ctx, C.c_void_p(d_scans[i].data_ptr()), d_scans[i].shape[0],
                                           fptr(inits[i])) == 0
    enqueue_round()
    torch.cuda.synchronize(dev)
    rounds = 6
    t1 = time.perf_counter()
    for _ in range(rounds):
        enqueue_round()
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t1
    # in-step: each scan's first correspondence launch inside its GN loop (a separate pass with stage timing)
    for o in ctxs:
        L.lo_set_stage_timing(o.ctx, 1)
    for _ in range(3):
        enqueue_round()
    tot_us = n_in = tot_ev = n_ev = 0.0
    for o in ctxs:
        us, cnt = C.c_double(0.0), C.c_int(0)
        assert L.lo_stage_span(o.ctx, C.byref(us), C.byref(cnt)) == 0
        tot_us += us.value * cnt.value
        n_in += cnt.value
        assert L.lo_stage_time(o.ctx, C.byref(us), C.byref(cnt)) == 0
        tot_ev += us.value * cnt.value
        n_ev += cnt.value
        L.lo_set_stage_timing(o.ctx, 0)
    in_t = tot_us / max(n_in, 1)
    in_ev = tot_ev / max(n_ev, 1)
    in_ach = float(np.mean(alg)) / (in_t * 1e-6) / 1e9 if in_t > 0 else None
    for o in ctxs:
        o.close()
    # DRAM bytes of one 1M-point launch (live rocprofv3 --pmc passes in child processes, as the value line's): a
    # 24 MB scan is far beyond the 4 MB L2 of an XCD, so isolated repeats of one scan miss L2 as the round-robin does
    traffic_live = None
    if pmc:
        keys, normals, cents, _ = vm.surfels()
        traffic_live = live_pmc({"pts": scans[0], "T": inits[0], "scale": it0[0][0], "alpha": it0[0][1], "keys": keys,
                                 "normals": normals, "centroids": cents, "voxel": 0.5}, reps=50)
        if traffic_live is not None:
            traffic_live["alg_bytes_per_launch"] = float(alg[0])
    return {"workload": "C5 synthetic 1M-point scans (1000 planar patches + 10 % outliers, azimuth order), "
                        f"{n_scans} distinct scans, one context each, round-robin on one stream",
            "value": rounds * n_scans / el, "unit": "scans/s (1M points)", "mode": mode, "gn_iters_per_scan_avg": float(np.mean(iters)),
            "working_set_bytes": float(ws), "in_cache": bool(ws <= MALL_BYTES), "map_surfels": vm.surfel_count(),
            "roofline": {"kernel": "k_correspond", "bound": "hbm", "achieved": rr_ach, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": rr_ach / HBM_PEAK_GBS, "kernel_us": rr_t,
                         "alg_bytes_per_launch": float(np.mean(alg)), "launches": rr_rounds * n_scans,
                         "traffic": traffic_live["hbm_bytes_per_launch"] if traffic_live else None,
                         "traffic_live": traffic_live,
                         "kernel_us_span": iso_t, "frac_span": iso_ach / HBM_PEAK_GBS,
                         "kernel_us_events_single": float(np.mean(iso_ev_us)) if iso_ev_us else None,
                         "timing": f"PRIMARY kernel_us: {rr_rounds} round-robin passes over the {n_scans} scans, every "
                                   "launch back to back with no set-up pass (each scan last touched "
                                   f"{n_scans - 1} launches earlier), HIP events around the whole sequence "
                                   "(lo_bench_correspond_rr): per-launch device time incl. the dispatch gap, what a "
                                   "rocprofv3 kernel trace of the leg reproduces; kernel_us_span = one launch's own span "
                                   "(first block's start to last block's end, s_memrealtime: no wave-launch ramp, no "
                                   "end-of-kernel drain); kernel_us_events_single = HIP events around single launches "
                                   "(adds the dispatch latency)"},
            "in_step": {"kernel_us": in_t, "achieved": in_ach, "frac": in_ach / HBM_PEAK_GBS if in_ach else None,
                        "scans": int(n_in), "kernel_us_events": in_ev,
                        "timing": "each scan's first correspondence launch inside its GN loop: its own span "
                                  "(lo_stage_span); kernel_us_events = HIP events around it (lo_stage_time)"}}


# --------------------------------------------------------------------------------------------------
# end to end: Estimator::process_frame loop (lo_odometry) over a raw sequence, frames/s
# --------------------------------------------------------------------------------------------------
def run_e2e(args, world, rank, local):
    import torch
    kd = args.config == "kitti_e2e_kdtree"
    from lidar_odometry_amd import synth
    from lidar_odometry_amd.odometry import LidarOdometry
    n_frames = 60
    seq = synth.KittiLikeSequence(seed=7 + rank, n_frames=n_frames, ramp_s=2.0)
    raws = [seq.scan(k) for k in range(n_frames)]
    torch.cuda.set_device(local)
    from lidar_odometry_amd import pinned_empty
    pinned = []                                               # scans as a sensor driver delivers them: pinned host
    for r in raws:                                            # buffers, read by the device filter in place
        a = pinned_empty(r.shape)
        a[:] = r
        pinned.append(a)

    def epoch(timed, scans=pinned):
        od = LidarOdometry(device=local, initial_pose=seq.poses[0], exact=args.mode == "exact",
                           use_surfel_correspondence=not kd)
        dt, poses, kf, dev_ms, map_ms = 0.0, [], 0, 0.0, 0.0
        try:
            for r in scans:
                t = time.perf_counter()
                T, info = od.process(r)
                dt += time.perf_counter() - t
                poses.append(T)
                kf += int(info.keyframe)
                dev_ms += info.device_ms
                map_ms += info.map_ms
        finally:
            od.close()
        return dt, poses, kf, dev_ms, map_ms

    epoch(False)                                              # warm-up (module load, allocations)
    n_ep = max(1, args.steps // n_frames)
    tot, kfs, dev, mp = 0.0, 0, 0.0, 0.0
    for _ in range(n_ep):
        dt, poses, kf, dev_ms, map_ms = epoch(True)
        tot += dt
        kfs += kf
        dev += dev_ms
        mp += map_ms
    frames = n_ep * n_frames
    if args.dump_outputs and rank == 0:                       # the last timed epoch's poses, one 3x4 per frame
        dump_outputs(args.dump_outputs, {"poses": np.stack([np.asarray(P, np.float32)[:3, :4] for P in poses])})
    if args.full:
        return run_e2e_full(args, world, rank, seq, raws, epoch, poses, n_frames, frames, tot, kfs, dev, mp, kd)
    return e2e_line(args, world, seq, raws, poses, n_frames, frames, tot, kfs, dev, mp, kd)


def e2e_line(args, world, seq, raws, poses, n_frames, frames, tot, kfs, dev, mp, kd):
    err = [float(np.linalg.norm(poses[k][:, 3] - seq.poses[k][:3, 3])) for k in range(n_frames)]
    return {
        "metric": METRIC + " (end to end: raw scan -> pose incl. keyframe map update)",
        "value": frames * world / tot, "unit": "frames/s", "n_gpus": world, "steps": frames, "warmup": n_frames,
        "ms_per_step": tot / frames * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (pose, J, H) + f64 (residuals, PKO)",
        "data": "synthetic raw HDL-64 sequence from rest (60 frames), raw scans in pinned host memory (lo_host_alloc)",
        "config": {"workload": "Estimator::process_frame loop (no loop closure / PGO), config/kitti.yaml, device filter + ICP, "
                               "device-resident VoxelMap update at keyframes (lo_devmap)" +
                               (", KDTree correspondences (RebuildKdTree as a device grid from the map's L0 centroids, "
                                "lo_devmap_sync_points)" if kd else ", surfel correspondences"),
                   "raw_points_per_frame_avg": float(np.mean([len(r) for r in raws])),
                   "keyframes_per_frame": kfs / frames, "parallelism": "single GPU per sequence",
                   "mode": args.mode, "mode_note": MODE_NOTE[args.mode]},
        "breakdown_ms_per_frame": {"device_filter_icp": dev / frames, "keyframe_map_update_host": mp / frames,
                                   "other_host": tot / frames * 1e3 - dev / frames - mp / frames},
        "translation_error_vs_gt_m_max": max(err),
    }


def run_e2e_full(args, world, rank, seq, raws, epoch, poses, n_frames, frames, tot, kfs, dev, mp, kd):
    """--full: the pageable-input and host-map A/B epochs, and the CPU restatement of the frame loop."""
    dt_pg, poses_pg, _, _, _ = epoch(True, raws)              # the same loop on pageable numpy scans (one staging copy)
    assert all(np.array_equal(a, b) for a, b in zip(poses_pg, poses)), "pinned and pageable inputs disagree"
    # A/B: the keyframe update on the host map + patch sync (LO_HOST_MAP=1) -- the same containers, so the same poses
    os.environ["LO_HOST_MAP"] = "1"
    try:
        dt_hm, poses_hm, kf_hm, _, map_hm = epoch(True)
    finally:
        del os.environ["LO_HOST_MAP"]
    assert all(np.array_equal(a, b) for a, b in zip(poses_hm, poses)), "device and host maps disagree"
    result = e2e_line(args, world, seq, raws, poses, n_frames, frames, tot, kfs, dev, mp, kd)
    result.update({
        "pageable_input_frames_per_s": n_frames / dt_pg,
        "host_map_ab": {"frames_per_s": n_frames / dt_hm, "keyframe_map_update_host_ms_per_frame": map_hm / n_frames,
                        "poses_bitwise_equal": True,
                        "what": "same loop with the host VoxelMap + patch sync at keyframes (LO_HOST_MAP=1)"},
    })
    if kd:                                                    # no CPU restatement of the KDTree frame loop: parity of
        result["parity"] = {"vs": "the same loop on the host map (host_map_ab, bitwise); the KDTree correspondence "
                                  "stage itself is bitwise vs the oracle in tests/test_gpu_kdtree.py"}   # this loop
    if rank == 0 and world == 1 and not args.no_cpu_baseline and not kd:
        import oracle
        t = time.perf_counter()
        n_cpu = 0
        ref_poses = None
        while time.perf_counter() - t < args.cpu_budget or ref_poses is None:
            rp, _ = oracle.odometry(raws, initial=seq.poses[0])
            if ref_poses is None:
                ref_poses = rp
            n_cpu += n_frames
        el = time.perf_counter() - t
        gp = np.stack([np.asarray(P, np.float32)[:3, :4].reshape(12) for P in poses])
        dtr = float(np.abs(gp.reshape(-1, 3, 4)[:, :, 3] - np.asarray(ref_poses).reshape(-1, 3, 4)[:, :, 3]).max())
        result["parity"] = {"frames": n_frames, "mode": args.mode,
                            "poses_bitwise_equal": int(sum(np.array_equal(a.view(np.uint32),
                                                                          np.asarray(b, np.float32).view(np.uint32))
                                                           for a, b in zip(gp, ref_poses))),
                            "max_abs_dt_m": dtr,
                            "vs": "oracle.odometry on the same raw scans (the CPU restatement of the frame loop)"}
        result["cpu_baseline"] = {"value": n_cpu / el, "unit": "frames/s", "cores": 1, "kind": "port",
                                  "sample": f"{n_cpu} frames ({n_cpu // n_frames} passes over the {n_frames}-frame sequence) "
                                            f"in {el:.1f} s, oracle.odometry (same loop on the CPU restatement)"}
        result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
    return result


# --------------------------------------------------------------------------------------------------
# loop-closure ICP: optimize_loop between two keyframes (IterativeClosestPointOptimizer.cpp:40-251), solves/s
# --------------------------------------------------------------------------------------------------
def run_loop(args, world, rank, local):
    import torch
    import oracle
    from lidar_odometry_amd import synth
    from lidar_odometry_amd.icp import IterativeClosestPointOptimizer
    seq = synth.KittiLikeSequence(seed=7, n_frames=42)
    rng = np.random.default_rng(900 + rank)
    pairs = []
    for fa in range(0, 36, 3):                                # keyframe fb re-observes fa with 0.3 m / 0.03 rad drift
        fb = fa + 3 + (fa // 3) % 2
        cur = oracle.voxel_filter(seq.scan(fb), 0.5, 8)
        mat = oracle.voxel_filter(seq.scan(fa), 0.5, 8)
        pairs.append((cur, pose12(synth.perturb(seq.poses[fb], rng, 0.3, 0.03)), mat, pose12(seq.poses[fa])))
    torch.cuda.set_device(local)
    icp = IterativeClosestPointOptimizer(device=local, max_points=max(len(p[0]) for p in pairs))
    icp.set_exact(args.mode == "exact")
    try:
        for k in range(max(args.warmup, len(pairs))):
            icp.optimize_loop(*pairs[k % len(pairs)])
        n_ok = n_it = 0
        t0 = time.perf_counter()
        for k in range(args.steps):
            ok, Tr, inl = icp.optimize_loop(*pairs[k % len(pairs)])
            n_ok += int(ok)
            n_it += icp.get_last_stats().num_iterations
        el = time.perf_counter() - t0
        if args.dump_outputs and rank == 0:                   # the last timed solve: success, T_rel, inlier ratio
            conv = Tr is not None
            dump_outputs(args.dump_outputs, {"relative_pose": Tr if conv else np.zeros((3, 4), np.float32),
                                             "status": np.array([float(ok), float(conv), inl if conv else 0.0])})
        gpu_res = []                                          # --full: the parity pass (after the timed region)
        for pr in pairs if args.full else []:
            ok, Tr, inl = icp.optimize_loop(*pr)
            st = icp.get_last_stats()
            gpu_res.append({"ok": bool(ok), "T": np.asarray(Tr if ok else np.zeros(12), np.float32).reshape(12).copy(),
                            "inlier": float(inl) if ok else None, "logs": st.iterations})
    finally:
        icp.close()
    result = {
        "metric": "loop-closure ICP solves/sec (optimize_loop: 5-NN plane fit, PKO, GN to convergence, inlier ratio)",
        "value": args.steps * world / el, "unit": "solves/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": el / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (pose, J, H) + f64 (plane fit, residuals, PKO)",
        "data": f"synthetic KITTI-like keyframe pairs ({len(pairs)}), host clouds in, relative pose out",
        "config": {"workload": "IterativeClosestPointOptimizer::optimize_loop between keyframes 3-4 frames apart, "
                               "config/kitti.yaml", "points_per_cloud_avg": float(np.mean([len(p[0]) for p in pairs])),
                   "gn_iters_per_solve": n_it / args.steps, "success_fraction": n_ok / args.steps,
                   "parallelism": "single GPU", "mode": args.mode, "mode_note": MODE_NOTE[args.mode]},
    }
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        t = time.perf_counter()
        n_cpu = 0
        while time.perf_counter() - t < args.cpu_budget or n_cpu < len(pairs):
            oracle.icp_optimize_loop(*pairs[n_cpu % len(pairs)])
            n_cpu += 1
        elc = time.perf_counter() - t
        result["cpu_baseline"] = {"value": n_cpu / elc, "unit": "solves/s", "cores": 1, "kind": "port",
                                  "sample": f"{n_cpu} optimize_loop solves over {len(pairs)} pairs in {elc:.1f} s "
                                            f"(oracle restatement, kd-tree 5-NN, single thread)"}
        ref = []
        for pr in pairs:
            ok_o, conv_o, Tr_o, inl_o, _, logs_o = oracle.icp_optimize_loop(*pr)
            ok_r = ok_o and conv_o
            ref.append({"ok": bool(ok_r), "T": np.asarray(Tr_o if ok_r else np.zeros(12), np.float32).reshape(12),
                        "inlier": inl_o if ok_r else None, "logs": logs_o})
        par = parity_vs_oracle(gpu_res, ref)
        par["bitwise_equal"] = parity_bitwise(gpu_res, ref)
        par["inlier_ratio_equal"] = sum(int(g["inlier"] == c["inlier"] or (g["inlier"] is not None and c["inlier"] is not None
                                                                         and np.float32(g["inlier"]) == np.float32(c["inlier"])))
                                        for g, c in zip(gpu_res, ref))
        par["mode"] = args.mode
        par["vs"] = "oracle.icp_optimize_loop on the same pairs: every GN iteration's pose, T_rel, status"
        result["cpu_baseline"]["parity"] = par
        result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
    return result


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n: int) -> int:
    """`--gpus N` without a launcher: start N rank processes of this script, one per GPU (RANK = LOCAL_RANK = r,
    WORLD_SIZE = N, rendezvous on 127.0.0.1), and return the worst exit code.  This parent never imports torch
    or touches the GPU, so no process that initialised HIP is ever replaced; the children inherit stdout, and only
    rank 0 prints the JSON line.  If one rank fails the others are terminated (they would wait in a barrier)."""
    import subprocess
    port = str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            c = p.poll()
            if c is None:
                continue
            live.remove(p)
            if c != 0 and rc == 0:
                rc = c
                log(f"[launcher] rank {procs.index(p)} exited with {c}; stopping the other ranks")
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    return rc


def check_gathered(gather, step: int, own: np.ndarray, rank: int, world: int, dist) -> dict:
    """The RCCL (or gloo) all-gathered records of `step` must hold every rank's own exported record in rank order:
    each rank contributes its own record through a separate object all-gather (host side, independent of the
    pipelined tensor collective) and every rank compares the two."""
    got = gather.records(step)
    mine = [None] * world
    dist.all_gather_object(mine, own.tolist())
    want = np.asarray(mine, np.float32).reshape(world, -1)
    ok = bool(np.array_equal(got, want))
    if not ok:
        raise RuntimeError(f"[rank {rank}] gathered pose records differ from the ranks' own records at step {step}:\n"
                           f"{got}\nvs\n{want}")
    return {"step": step, "ranks": world, "records_equal": ok,
            "statuses": [int(x) for x in got[:, 12]], "iterations": [int(x) for x in got[:, 13]]}


def run_dry(args, world, rank):
    """`--dry-run`: the launcher / rendezvous / gather / timing plumbing on CPU (gloo) with NO ICP: each step's
    record is the step's initial pose with the rank and step in the status fields.  For rehearsing `--gpus N` where
    no GPU exists; the line says so and carries no throughput claim about the ICP."""
    import torch
    import torch.distributed as dist
    from lidar_odometry_amd.parallel import PipelinedPoseGather
    if world > 1:
        dist.init_process_group(backend="gloo")
    gather = PipelinedPoseGather(world, None)
    rng = np.random.default_rng(rank)
    own = None

    def step(k):
        nonlocal own
        r = gather.slot()
        rec = np.zeros(16, np.float32)
        rec[:12] = rng.standard_normal(12)
        rec[12], rec[13], rec[14] = 0.0, float(k % 4 + 1), float(rank)
        r.copy_(torch.from_numpy(rec))
        own = rec
        gather.launch()

    for k in range(args.warmup):
        step(k)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(args.warmup + k)
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    els = [el]
    chk = None
    if args.dump_outputs and rank == 0 and own is not None:
        dump_outputs(args.dump_outputs, {"record": own})
    if world > 1:
        gather.drain()
        chk = check_gathered(gather, args.warmup + args.steps - 1, own, rank, world, dist)
        els = [None] * world
        dist.all_gather_object(els, el)
        el = max(els)
    res = {"metric": "bench.py --dry-run (launcher / gather plumbing only, no ICP)", "value": args.steps * world / el,
           "unit": "records/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic records",
           "config": {"workload": "dry run: pose-record all-gather over gloo", "parallelism": f"x{world} ranks"},
           "per_rank_s": els, "gather_check": chk}
    if world > 1:
        dist.destroy_process_group()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks (one per GPU); without WORLD_SIZE in the environment this process spawns them")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend for the pose gather (nccl = RCCL; gloo moves the records through host "
                         "memory, e.g. to rehearse N ranks sharing one GPU)")
    ap.add_argument("--dry-run", action="store_true", help="CPU plumbing rehearsal without ICP (see run_dry)")
    ap.add_argument("--check-records", action="store_true",
                    help="diagnostic: keep every step's pose record and compare its iteration count with the pre-pass")
    ap.add_argument("--data-rank", type=int, default=None, help="diagnostic: build the workload of this rank")
    ap.add_argument("--steps", type=int, default=1000, help="timed steps")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement and check (spread passes, per-kernel times, rooflines, "
                         "live PMC, pipeline off, other mode, PCIe-inclusive, multi-sequence, batched, C5, CPU baseline "
                         "and parity); a plain run only times the steps")
    ap.add_argument("--full-budget", type=float, default=330.0,
                    help="--full: seconds after which the batched sizes still to come and the C5 leg are skipped (named "
                         "in the line); a run on an idle MI355X needs about 120 s beside its timed steps")
    ap.add_argument("--spread-passes", type=int, default=7,
                    help="extra back-to-back passes of the timed K steps whose min / median / max go to value_spread")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--config", default="kitti", choices=sorted(WORKLOADS) + ["kitti_e2e", "kitti_e2e_kdtree", "kitti_loop"])
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of oracle CPU work for cpu_baseline")
    ap.add_argument("--c5", type=int, default=12,
                    help="extra measurement with --config kitti: this many distinct 1M-point scans (C5), one context "
                         "each, rotated so each launch reads its scan from HBM; 0 = skip")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mode", default="exact", choices=["exact", "fast", "auto", "default"],
                    help="arithmetic order of the timed GN step: exact (the library's default) = the reference's own "
                         "fp32 order (sequential sums, fp32 LDLT, JacobiSVD SO3; bit-identical to the oracle), fast = "
                         "fp64 tree sums + fp64 solve (lo_set_exact(ctx, 0): within ~1e-7 per step, but a near-tie in "
                         "the PKO's JS argmin can flip alpha; 'default' is its old name); auto = fast when, on EVERY "
                         "rank, its every iteration on the workload's scans is within the north_star's 1e-4 m / 1e-4 "
                         "rad of the oracle, else exact.  The other mode is timed beside it as other_mode")
    ap.add_argument("--order", default="azimuth", choices=["azimuth", "random"], help="patch1m scan point order")
    ap.add_argument("--sequences", type=int, default=8,
                    help="extra measurement: independent sequences sharing this GPU, one context + HIP stream each "
                         "(0 = skip); reported as multi_sequence, never as value")
    ap.add_argument("--pmc", default="live", choices=["live", "off"],
                    help="HBM traffic of the roofline kernel: live rocprofv3 --pmc passes in child processes (rank 0, "
                         "1 GPU), or off (the committed profiles/pmc_traffic.json figure)")
    ap.add_argument("--pmc-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=str, default="64,256,1024,2048,4096",
                    help="extra measurement: comma list of B for the scan-parallel batch (lo_batch_*: B independent "
                         "contexts advanced in lockstep, one launch per kernel per GN iteration); '' = skip; "
                         "reported as batched, never as value")
    args = ap.parse_args()
    if args.mode == "default":
        args.mode = "fast"
    global ORDER
    ORDER = args.order
    if args.pmc_child:
        pmc_child(args.pmc_child)

    if args.gpus < 1:
        sys.exit(f"--gpus must be >= 1 (got {args.gpus})")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    _claim_stdout()
    if world != args.gpus:
        sys.exit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}; refusing to report a {args.gpus}-GPU line "
                 f"from {world} rank(s)")
    if args.dry_run:
        res = run_dry(args, world, rank)
        if rank == 0:
            emit(res)
        return
    import torch
    import torch.distributed as dist
    # one rank per GPU; more ranks than GPUs (a rehearsal on a small box) wrap around
    local %= max(1, torch.cuda.device_count())
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend="gloo")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    if args.config in ("kitti_e2e", "kitti_e2e_kdtree", "kitti_loop"):
        if args.mode == "auto":           # the frame loop and the loop-closure solve: reference-exact arithmetic
            args.mode = "exact"
        result = (run_loop if args.config == "kitti_loop" else run_e2e)(args, world, rank, local)
        if rank == 0:
            emit(result)
        if world > 1:
            dist.destroy_process_group()
        return

    from lidar_odometry_amd import lib
    from lidar_odometry_amd.icp import AdaptiveMEstimatorConfig, ICPConfig, IterativeClosestPointOptimizer, MapGeometry

    t_data = time.perf_counter()
    wl = WORKLOADS[args.config](rank if args.data_rank is None else args.data_rank)
    log(f"[rank {rank}] data built in {time.perf_counter() - t_data:.1f} s: {len(wl['scans'])} scans, "
        f"avg {np.mean([len(s) for s in wl['scans']]):.0f} pts, {wl['vm'].surfel_count()} surfels")
    max_pts = max(len(s) for s in wl["scans"])
    raw = bool(wl.get("raw", False))
    if raw:
        max_pts = max(max_pts, max((len(r) + 7) // 8 for r in wl["raw_scans"]))
    kd = bool(wl.get("kdtree", False))
    icp = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=not kd), AdaptiveMEstimatorConfig(),
                                         MapGeometry(voxel_size=wl["voxel"]), device=local, max_points=max_pts)
    L = lib()
    mode_selection = None
    if args.mode == "auto":
        # the north_star's bar decides the reported mode: default arithmetic only when every iteration of every scan of
        # this workload is within 1e-4 m / 1e-4 rad of the oracle (and keeps its iteration count and status)
        assert L.lo_map_set_from_voxelmap(icp.ctx, wl["vm"].handle) == 0
        t_sel = time.perf_counter()
        ref_sel = oracle_reference(wl)
        icp.set_exact(False)
        sel = []
        for i in range(len(wl["scans"])):
            ok, To = icp.optimize(None, wl["scans"][i], pose12(wl["inits"][i]))
            sel.append({"ok": bool(ok), "T": np.asarray(To, np.float32).reshape(12).copy(),
                        "logs": icp.get_last_stats().iterations})
        p_sel = parity_vs_oracle(sel, ref_sel)
        passes = bool(p_sel["within_1e-4"] and p_sel["iteration_count_equal"] == p_sel["scans"]
                      and p_sel["status_equal"] == p_sel["scans"])
        # every rank decides on its own scans; all ranks time the same mode (all-reduce MIN of the verdicts)
        from lidar_odometry_amd.parallel import all_ranks_agree
        agreed = all_ranks_agree(passes, world, None if (world == 1 or args.dist_backend == "gloo") else dev)
        args.mode = "fast" if agreed else "exact"
        mode_selection = {"rule": "fast arithmetic when, on every rank, its every iteration on that rank's scans is "
                                  "within 1e-4 m / 1e-4 rad of the oracle with equal iteration counts and status, else "
                                  "reference-exact", "fast_parity": p_sel, "this_rank_passes": passes,
                          "all_ranks_pass": agreed, "chosen": args.mode, "seconds": time.perf_counter() - t_sel}
        log(f"[rank {rank}] mode auto -> {args.mode} (fast within 1e-4 here: {p_sel['within_1e-4']}, all ranks: {agreed})")
    icp.set_exact(args.mode == "exact")
    other = "fast" if args.mode == "exact" else "exact"
    # one stream shared by the ICP context and torch (pose-record copies, the gather's events): a dedicated stream,
    # because handle 0 (torch's legacy default stream) means "the context's own non-blocking stream" to
    # lo_set_stream, which the default stream does not order against
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    L.lo_set_stream(icp.ctx, C.c_void_p(stream.cuda_stream))
    rc = L.lo_map_set_from_voxelmap(icp.ctx, wl["vm"].handle)
    assert rc == 0, rc
    d_scans = [torch.from_numpy(s).to(dev) for s in wl["scans"]]
    d_raw = [torch.from_numpy(r).to(dev) for r in wl["raw_scans"]] if raw else None
    inits = [pose12(T) for T in wl["inits"]]
    fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    from lidar_odometry_amd.parallel import PipelinedPoseGather
    # scan-parallel replicas: the only collective is the per-step pose all-gather (RCCL), on a side stream
    gloo = world > 1 and args.dist_backend == "gloo"
    gather = PipelinedPoseGather(world, None if gloo else dev)
    dev_rec = torch.zeros(16, dtype=torch.float32, device=dev)
    # --check-records: every step's exported record kept on the device (diagnostic; adds one tiny launch per step)
    rec_log = torch.zeros(args.warmup + args.steps, 16, dtype=torch.float32, device=dev) if args.check_records else None
    n_step = [0]

    def step(k):
        i = k % len(d_scans)
        if raw:
            rc = L.lo_icp_optimize_raw_async(icp.ctx, C.c_void_p(d_raw[i].data_ptr()), d_raw[i].shape[0], 8,
                                             C.c_float(0.5), fptr(inits[i]))
        else:
            rc = L.lo_icp_optimize_async(icp.ctx, C.c_void_p(d_scans[i].data_ptr()), d_scans[i].shape[0], fptr(inits[i]))
        if rc != 0:
            raise RuntimeError(f"lo_icp_optimize_async rc={rc}: {L.lo_last_error(icp.ctx).decode()}")
        if world > 1:
            if gloo:                                  # host-memory collective: D2H of the record, then gloo
                L.lo_icp_export_pose(icp.ctx, C.c_void_p(dev_rec.data_ptr()))
                gather.slot().copy_(dev_rec)
            else:                                     # RCCL on the side stream, off the critical path
                L.lo_icp_export_pose(icp.ctx, C.c_void_p(gather.slot().data_ptr()))
            gather.launch()
        if rec_log is not None and n_step[0] < rec_log.shape[0]:      # the warmup + timed steps (later passes: no log)
            L.lo_icp_export_pose(icp.ctx, C.c_void_p(rec_log[n_step[0]].data_ptr()))
        n_step[0] += 1

    # per-scan GN iteration counts + accuracy vs ground truth (deterministic, so the timed pass repeats them); the
    # results are also compared with the oracle's in cpu_baseline (parity of the measured workload itself)
    iters, errs, gpu_res = [], [], []
    for i in range(len(d_scans)):
        ok, To = icp.optimize(None, wl["scans"][i], inits[i])
        st = icp.get_last_stats()
        iters.append(st.num_iterations)
        errs.append(float(np.linalg.norm(To[:, 3] - wl["gts"][i][:3, 3])))
        gpu_res.append({"ok": bool(ok), "T": np.asarray(To, np.float32).reshape(12).copy(), "logs": st.iterations})
    # --full: algorithmic bytes of each scan's first correspondence pass at its initial pose (formula: see alg_bytes
    # below)
    scan_alg_bytes = []
    for i in range(len(d_scans) if args.full else 0):
        nv_i, _, _ = icp.find_correspondences(wl["scans"][i], inits[i])
        ni = len(wl["scans"][i])
        scan_alg_bytes.append(ni * (12 + 80 + 40 + 4 + 0.125) + 40 * nv_i if kd else ni * (12 + 8 + 4 + 8 + 0.125) + 24 * nv_i)
    L.lo_set_stream(icp.ctx, C.c_void_p(stream.cuda_stream))
    for k in range(args.warmup):
        step(k)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, icp_result_arrays(L, icp))
    if rec_log is not None:
        recs = rec_log.cpu().numpy()
        ks = list(range(args.warmup)) + list(range(args.steps))
        bad = [(j, ks[j] % len(iters), int(recs[j, 13]), iters[ks[j] % len(iters)]) for j in range(len(ks))
               if int(recs[j, 13]) != iters[ks[j] % len(iters)]]
        log(f"[rank {rank}] record check: {len(bad)} of {len(ks)} steps differ from the pre-pass iteration counts; "
            f"first: {bad[:8]}")
    per_rank = [el]
    gather_check = None
    if world > 1:
        gather.drain()
        last = args.warmup + args.steps - 1
        own = gather.recs[last % gather.depth].detach().cpu().numpy()
        # this rank's own record of the last step, exported by the ICP context, against the collective's result
        want_it = iters[(args.steps - 1) % len(iters)]           # the last timed step ran scan (steps-1) % n
        assert int(own[13]) == want_it, (own, want_it)
        gather_check = check_gathered(gather, last, own, rank, world, dist)
        per_rank = [None] * world
        dist.all_gather_object(per_rank, el)
        el = max(per_rank)
    total_scans = args.steps * world
    total_iters = sum(iters[k % len(iters)] for k in range(args.steps)) * world
    result = {
        "metric": METRIC,
        "value": total_scans / el,
        "unit": "scans/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": el / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32 (pose, J, H) + f64 (residuals, PKO)",
        "data": "synthetic (deterministic raycast scenes; no dataset reachable offline)",
        "config": {"workload": wl["name"], "points_per_scan_avg": float(np.mean([len(s) for s in wl["scans"]])),
                   **({"raw_points_per_scan_avg": float(np.mean([len(r) for r in wl["raw_scans"]]))} if raw else {}),
                   "distinct_scans": len(wl["scans"]), "map_surfels": wl["vm"].surfel_count(),
                   "map_l0_points": wl["vm"].l0_count(), "correspondence": "kdtree 5-NN" if kd else "L1 surfel",
                   "max_iterations": 4, "gn_iters_per_scan_avg": float(np.mean(iters)),
                   "parallelism": (f"scan-parallel x{world} (pose all-gather per step over "
                                   f"{'gloo, host memory' if gloo else 'RCCL, side stream'})") if world > 1
                   else "single GPU: context stream + tail stream (scan pipeline)",
                   "mode": args.mode, "mode_note": MODE_NOTE[args.mode], "mode_selection": mode_selection},
        "gn_iters_per_sec": total_iters / el,
        "per_rank": None if world == 1 else {"scans_per_s": [args.steps / e for e in per_rank], "timed_s": per_rank,
                                             "backend": args.dist_backend, "gather_check": gather_check},
        "translation_error_vs_gt_m_median": float(np.median(errs)),
    }
    if not args.full:                       # a plain run: the timed steps and their line, nothing else
        icp.close()
        if rank == 0:
            emit(result)
        if world > 1:
            dist.destroy_process_group()
        return

    # ---- everything below: --full only ----
    # the spread of the timed window: the same K steps timed again several times back to back, so a
    # short driver window's value can be read against its run-to-run variation (`value` stays the single pass above)
    value_spread = None
    if world == 1 and rec_log is None and args.spread_passes > 0:
        rates = []
        n_sp = min(args.steps, 5000)
        for _ in range(args.spread_passes):
            torch.cuda.synchronize(dev)
            t_p = time.perf_counter()
            for k in range(n_sp):
                step(k)
            torch.cuda.synchronize(dev)
            rates.append(n_sp / (time.perf_counter() - t_p))
        rates.sort()
        value_spread = {"passes": len(rates), "steps_per_pass": n_sp, "min": rates[0],
                        "median": float(np.median(rates)), "max": rates[-1], "unit": "scans/s",
                        "note": "the timed K steps (at most 5000 of them, so that a long timed window does not "
                                "multiply the run time) repeated back to back after the value pass (same scans, same "
                                "warm state); value is the single pass before them"}

    # live per-kernel device times (HIP events around back-to-back launches on this context's stream)
    i0 = int(np.argmax([len(s) for s in wl["scans"]]))
    # the scan's own iteration-0 normalisation scale and PKO alpha, so the isolated launches see the real
    # residual distribution (EM iteration count) and weights
    icp.optimize(None, wl["scans"][i0], inits[i0])
    it0 = icp.get_last_stats().iterations
    scale0 = float(it0[0]["scale"]) if it0 else 0.01
    alpha0 = float(it0[0]["alpha"]) if it0 else 1.0
    kern_us = {}
    stage0 = "k_knn+k_knn_brute+k_plane" if kd else "k_correspond"
    for kid, name in enumerate((stage0, "k_accumulate", "k_pko", "k_solve")):
        ms = C.c_float(0.0)
        reps = 200 if kid != 2 else 50
        rc = L.lo_bench_kernel(icp.ctx, C.c_void_p(d_scans[i0].data_ptr()), d_scans[i0].shape[0], fptr(inits[i0]),
                               C.c_double(scale0), C.c_double(alpha0), kid, reps, C.byref(ms))
        assert rc == 0, rc
        kern_us[name] = ms.value * 1e3
    # in-step duration of each scan's first correspondence launch (HIP events on the context stream around that
    # launch inside the real GN loop), over a separate pass of the same steps (events would perturb the timed pass)
    n_in = min(args.steps, 200)
    em0 = (C.c_ulonglong * 3)()
    assert L.lo_pko_em_stats(icp.ctx, em0, 1) == 0               # zero the EM clock sums
    L.lo_set_stage_timing(icp.ctx, 1)
    in_bytes = 0.0
    for k in range(n_in):
        i = k % len(d_scans)
        if raw:
            rc = L.lo_icp_optimize_raw_async(icp.ctx, C.c_void_p(d_raw[i].data_ptr()), d_raw[i].shape[0], 8,
                                             C.c_float(0.5), fptr(inits[i]))
        else:
            rc = L.lo_icp_optimize_async(icp.ctx, C.c_void_p(d_scans[i].data_ptr()), d_scans[i].shape[0], fptr(inits[i]))
        assert rc == 0, rc
        in_bytes += scan_alg_bytes[i]
    in_us, in_cnt = C.c_double(0.0), C.c_int(0)
    assert L.lo_stage_time(icp.ctx, C.byref(in_us), C.byref(in_cnt)) == 0
    L.lo_set_stage_timing(icp.ctx, 0)
    # the dominant kernel (k_pko_t) measured in the same pass: the lead workgroup clocks its EM loop (s_memtime)
    em = (C.c_ulonglong * 3)()
    assert L.lo_pko_em_stats(icp.ctx, em, 1) == 0
    em_live = {"cycles_per_em_iteration": em[0] / em[1] if em[1] else None,
               "em_iterations_per_fit": em[1] / em[2] if em[2] else None, "fits": int(em[2]),
               "scans": in_cnt.value,
               "timing": "s_memtime around the EM loop of the lead PKO workgroup, inside the GN loop of this pass"}
    n0 = d_scans[i0].shape[0]
    n_valid, valid, _ = icp.find_correspondences(wl["scans"][i0], inits[i0])
    v = n_valid / n0
    # algorithmic bytes per k_correspond launch: per point 12 B point + 8 B key probe + 24 B payload on a hit
    # (lower-bounded by the accepted fraction v) + 4 B slot index and 8 B fp64 residual written (the PKO sample
    # reads the residual back) + 1/8 B validity ballot
    alg_bytes = n0 * (12 + 8 + 24 * v + 4 + 8 + 0.125)
    corr_kernel = "k_correspond"
    if kd:
        # KDTree stage (k_knn + k_knn_brute + k_plane): per point 12 B point + 5 x 16 B neighbour centroids +
        # 20 B neighbour list written and re-read + 4 B slot; per accepted point 32 B plane + 8 B residual
        alg_bytes = n0 * (12 + 80 + 40 + 4 + 0.125 + 40 * v)
        corr_kernel = stage0
    t_corr = kern_us[stage0] * 1e-6
    ws_bytes = float(n0 * (12 + 4 + 32))
    achieved = alg_bytes / t_corr / 1e9
    traffic = read_pmc_traffic(args.config + ("_random" if args.config == "patch1m" and ORDER == "random" else ""))
    traffic_source = "profiles/pmc_traffic.json (separate rocprofv3 --pmc passes, earlier run)"
    traffic_live = None
    if not kd and rank == 0 and world == 1 and args.pmc == "live":
        keys, normals, cents, _ = wl["vm"].surfels()
        traffic_live = live_pmc({"pts": wl["scans"][i0], "T": inits[i0], "scale": scale0, "alpha": alpha0,
                                 "keys": keys, "normals": normals, "centroids": cents, "voxel": wl["voxel"]})
        if traffic_live is not None:
            traffic = traffic_live["hbm_bytes_per_launch"]
            traffic_source = ("live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this run (child processes, "
                              "200 isolated launches of the same scan and map)")
    # where a step's device time goes: isolated kernel time x launches per scan (working launches only)
    gi = float(np.mean(iters))
    # small scans with PKO (<= 64 accumulate blocks): the accumulate runs inside the k_pko launch (one candidate
    # per alpha, off the critical path; kern_us["k_pko"] includes it) and a one-workgroup k_solve_pick solves
    spec = bool(icp.adaptive.use_adaptive_m_estimator) and (n0 + 255) // 256 <= 64
    per_scan = {k: v * gi for k, v in kern_us.items() if not (spec and k == "k_accumulate")}
    dom = max(per_scan, key=per_scan.get)

    # the scan pipeline (lo_set_pipeline, on by default and in `value`): the same steps with it switched off, so the
    # line shows what the tail stream buys (results are bit-identical either way: tests/test_gpu_pipeline.py)
    pipeline = {"main_iterations": int(os.environ.get("LO_PIPE_MAIN", "2")),
                "enabled": os.environ.get("LO_PIPE", "1") != "0",
                "note": "GN iterations >= main_iterations of a small PKO scan run on the context's tail stream; the "
                        "context stream is held on the device (k_wait_final) only until the scan's result is final"}
    if world == 1 and pipeline["enabled"] and rec_log is None:
        n_po = min(args.steps, 1000)
        L.lo_set_pipeline(icp.ctx, 0, 0)
        for k in range(10):
            step(k)
        torch.cuda.synchronize(dev)
        t5 = time.perf_counter()
        for k in range(n_po):
            step(k)
        torch.cuda.synchronize(dev)
        pipeline["value_pipeline_off"] = n_po / (time.perf_counter() - t5)
        pipeline["steps_pipeline_off"] = n_po
        L.lo_set_pipeline(icp.ctx, 1, 0)

    # PCIe-inclusive rate (never `value`): lo_icp_optimize on HOST buffers = H2D points, the same device
    # GN loop, D2H pose + per-iteration logs and a stream sync per scan
    n_pc = min(200, max(20, args.steps // 5))
    t1 = time.perf_counter()
    for k in range(n_pc):
        i = k % len(d_scans)
        icp.optimize(None, wl["scans"][i], inits[i])
    pcie_rate = n_pc / (time.perf_counter() - t1)

    # the other arithmetic mode (exact <-> default): the same steps timed, and every scan's result kept for the parity
    # comparison with the oracle (cpu_baseline.parity_other)
    icp.set_exact(other == "exact")
    gpu_other = []
    for i in range(len(d_scans)):
        ok, To = icp.optimize(None, wl["scans"][i], inits[i])
        st = icp.get_last_stats()
        gpu_other.append({"ok": bool(ok), "T": np.asarray(To, np.float32).reshape(12).copy(), "logs": st.iterations})
    L.lo_set_stream(icp.ctx, C.c_void_p(stream.cuda_stream))
    n_ot = min(args.steps, 300)
    for k in range(10):
        step(k)
    torch.cuda.synchronize(dev)
    t4 = time.perf_counter()
    for k in range(n_ot):
        step(k)
    torch.cuda.synchronize(dev)
    el4 = time.perf_counter() - t4
    icp.set_exact(args.mode == "exact")
    other_mode = {"mode": other, "value": n_ot / el4, "unit": "scans/s", "steps": n_ot,
                  "gn_iters_per_sec": sum(len(gpu_other[k % len(gpu_other)]["logs"]) for k in range(n_ot)) / el4,
                  "mode_note": MODE_NOTE[other],
                  "note": "the other arithmetic mode, timed like value (never value); parity in cpu_baseline.parity_other"}

    # independent sequences sharing the GPU (serving many sensors / logs): B contexts, one HIP stream each,
    # scans enqueued round-robin without host syncs; aggregate scans/s.  Never `value`.
    multi = None
    B = args.sequences if (world == 1 and not kd) else 0
    if B > 1:
        ctxs = [icp] + [IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=not kd), AdaptiveMEstimatorConfig(),
                                                       MapGeometry(voxel_size=wl["voxel"]), device=local, max_points=max_pts)
                        for _ in range(B - 1)]
        for o in ctxs[1:]:
            o.set_exact(args.mode == "exact")
        L.lo_set_stream(icp.ctx, None)                  # back to the context's own stream
        for o in ctxs[1:]:
            assert L.lo_map_set_from_voxelmap(o.ctx, wl["vm"].handle) == 0
        K2 = max(50, min(args.steps, 400))

        def enqueue(k):
            for b, o in enumerate(ctxs):
                i = (k + 7 * b) % len(d_scans)
                if raw:
                    rc = L.lo_icp_optimize_raw_async(o.ctx, C.c_void_p(d_raw[i].data_ptr()), d_raw[i].shape[0], 8,
                                                     C.c_float(0.5), fptr(inits[i]))
                else:
                    rc = L.lo_icp_optimize_async(o.ctx, C.c_void_p(d_scans[i].data_ptr()), d_scans[i].shape[0],
                                                 fptr(inits[i]))
                assert rc == 0, rc
        for k in range(10):
            enqueue(k)
        for o in ctxs:
            L.lo_sync(o.ctx)
        t2 = time.perf_counter()
        for k in range(K2):
            enqueue(k)
        for o in ctxs:
            L.lo_sync(o.ctx)
        el2 = time.perf_counter() - t2
        multi = {"sequences": B, "value": B * K2 / el2, "unit": "scans/s", "steps_per_sequence": K2, "mode": args.mode,
                 "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
                 "note": "independent scan streams, one context + HIP stream each; aggregate throughput, not value"}
        for o in ctxs[1:]:
            o.close()

    # scan-parallel batch on this GPU: B independent contexts (own map copy, scan and GN state each), one launch
    # per kernel per GN iteration for all B (lo_batch_*).  Aggregate scans/s of B sequences; never `value`.
    batched = None
    sizes = [int(x) for x in args.batch.split(",") if x.strip()] if (world == 1 and not kd and not raw) else []
    if sizes:
        from lidar_odometry_amd import BatchOptimizer
        from lidar_odometry_amd._lib import LoBatchRec
        batched = {"unit": "scans/s", "runs": [], "mode": args.mode, "mode_note": MODE_NOTE[args.mode],
                   "note": "B independent sequences on one GPU (one context each: own map copy, scan, GN state), "
                           "advanced in lockstep by lo_batch_optimize_async; aggregate throughput, not value"}
        pool = []
        # per distinct scan: algorithmic bytes of one correspondence pass at its initial pose (as alg_bytes above)
        scan_bytes = []
        for i in range(len(d_scans)):
            nv, _, _ = icp.find_correspondences(wl["scans"][i], inits[i])
            scan_bytes.append(len(wl["scans"][i]) * (12 + 8 + 4 + 8 + 0.125) + 24 * nv)
        def new_job_ctx():
            o = IterativeClosestPointOptimizer(ICPConfig(), AdaptiveMEstimatorConfig(), MapGeometry(voxel_size=wl["voxel"]),
                                               device=local, max_points=max_pts)
            o.set_exact(args.mode == "exact")
            assert L.lo_map_set_from_voxelmap(o.ctx, wl["vm"].handle) == 0
            return o
        # device memory per job context, measured: the free-memory drop over a few contexts that have
        # each run one optimize (so every lazily allocated buffer exists), plus the job's private scan copy; sizes
        # whose contexts would not fit in 80 % of the free HBM left are skipped (named in the line)
        torch.cuda.synchronize(dev)
        free0 = torch.cuda.mem_get_info(dev)[0]
        n_probe = 8
        for _ in range(n_probe):
            pool.append(new_job_ctx())
            pool[-1].optimize(None, wl["scans"][0], inits[0])
        torch.cuda.synchronize(dev)
        free1 = torch.cuda.mem_get_info(dev)[0]
        per_ctx = max((free0 - free1) / n_probe, float(1 << 20)) + 12.0 * max_pts
        cap_b = n_probe + int(0.8 * free1 // per_ctx)
        batched["per_context_bytes_measured"] = per_ctx
        skipped = [B for B in sizes if B > cap_b]
        sizes = [B for B in sizes if B <= cap_b]
        if skipped:
            batched["skipped_sequences"] = skipped
            batched["skipped_note"] = (f"{per_ctx / 2**20:.1f} MB of device buffers per context (measured): {cap_b} "
                                       "contexts fit")
        for B in sizes:
            if over_budget(args):                     # a slow host: the remaining sizes are named, not run
                batched.setdefault("skipped_for_time", []).append(B)
                log(f"[batch] B={B}: skipped, the run is past --full-budget ({args.full_budget:.0f} s)")
                continue
            while len(pool) < B:
                pool.append(new_job_ctx())
            bo = BatchOptimizer(pool[:B])
            K3 = max(20, min(args.steps // 4, 100))
            # the C ABI directly (what a C++ caller does): per distinct step, the device pointers, counts and
            # initial poses are prepared once; the timed loop is enqueue + wait, records into a fixed array
            nd = len(d_scans)
            # job j's scan: a private device copy of distinct scan j % nd (B separate buffers, as B sensors have;
            # every job also has its own map copy), optimized from its initial pose each batch
            sel = [j % nd for j in range(B)]
            job_scans = [d_scans[i].clone() for i in sel]
            c_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in job_scans])
            c_cnts = (C.c_size_t * B)(*[t.shape[0] for t in job_scans])
            c_T = np.ascontiguousarray(np.stack([inits[i] for i in sel]))
            recs = (LoBatchRec * B)()
            ms = C.c_double(0.0)

            def batch_step(k):
                rc = L.lo_batch_optimize_async(bo._b, c_ptrs, c_cnts, fptr(c_T))
                rc2 = L.lo_batch_result(bo._b, recs, C.byref(ms))
                if rc != 0 or rc2 != 0:
                    raise RuntimeError(f"lo_batch rc={rc}/{rc2}: {L.lo_batch_last_error(bo._b).decode()}")
                return ms.value
            for k in range(5):
                batch_step(k)
            dev_ms = []
            t3 = time.perf_counter()
            for k in range(K3):
                dev_ms.append(batch_step(k))
            el3 = time.perf_counter() - t3
            n_it = sum(iters[i] for i in sel) * K3
            ok = sum(r.status == 0 for r in recs)
            batched["runs"].append({"sequences": B, "value": B * K3 / el3, "gn_iters_per_sec": n_it / el3,
                                    "batches": K3, "ms_per_batch": el3 / K3 * 1e3,
                                    "device_ms_per_batch": float(np.mean(dev_ms)), "ok_last_batch": int(ok)})
            # batched correspondence kernel vs the HBM roofline: algorithmic bytes of all B jobs per launch
            cms = C.c_float(0.0)
            assert L.lo_batch_optimize_async(bo._b, c_ptrs, c_cnts, fptr(c_T)) == 0
            assert L.lo_batch_result(bo._b, recs, C.byref(ms)) == 0
            if L.lo_batch_bench_correspond(bo._b, 50, C.byref(cms)) != 0:
                # no job ran in lockstep: reference-exact jobs beyond 8192 points run their own exact GN loops
                batched["runs"][-1]["roofline"] = None
                batched["runs"][-1]["lockstep"] = False
                del job_scans
                log(f"[batch] B={B}: {B * K3 / el3:.0f} scans/s (exact jobs beyond 8192 points: not in lockstep)")
                bo.close()
                continue
            bbytes = sum(scan_bytes[i] for i in sel)
            npts = int(sum(d_scans[i].shape[0] for i in sel))
            ach = bbytes / (cms.value * 1e-3) / 1e9
            wsb = float(npts * (12 + 4 + 32))
            batched["runs"][-1]["roofline"] = {"kernel": "k_correspond_b", "bound": "hbm", "achieved": ach,
                                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                                               "kernel_us": cms.value * 1e3, "alg_bytes_per_launch": bbytes,
                                               "points_per_launch": npts, "working_set_bytes": wsb,
                                               "in_cache": wsb <= MALL_BYTES,
                                               "traffic": read_pmc_traffic(f"{args.config}_batch{B}")}
            if args.pmc == "live" and B == sizes[-1]:
                # the largest batch (beyond the 256 MB Infinity Cache at B >= 2048): HBM traffic measured live
                keys, normals, cents, _ = wl["vm"].surfels()
                case = {"batch": B, "n_scans": nd, "inits": np.stack(inits), "keys": keys, "normals": normals,
                        "centroids": cents, "voxel": wl["voxel"]}
                for i in range(nd):
                    case[f"scan_{i}"] = wl["scans"][i]
                tl = live_pmc(case, reps=50, kernel="k_correspond_b")
                if tl is not None:
                    batched["runs"][-1]["roofline"]["traffic"] = tl["hbm_bytes_per_launch"]
                    batched["runs"][-1]["roofline"]["traffic_live"] = tl
            del job_scans
            log(f"[batch] B={B}: {B * K3 / el3:.0f} scans/s, {el3 / K3 * 1e3:.3f} ms/batch "
                f"(device {np.mean(dev_ms):.3f} ms)")
            bo.close()
        batched["value"] = max((r["value"] for r in batched["runs"]), default=None)
        if rank == 0 and not args.no_cpu_baseline:
            thr = max(1, min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
            batched["cpu_baseline"] = cpu_baseline_replicas(wl, args.cpu_budget / 2, thr)
            batched["speedup_vs_cpu_replicas"] = (batched["value"] / batched["cpu_baseline"]["value"]
                                                  if batched["value"] else None)
        for o in pool:
            o.close()

    result.update({
        "value_spread": value_spread,
        "pipeline": pipeline,
        "kernel_us": kern_us,
        "step_device_us_est": {"per_kernel": per_scan, "dominant_kernel": dom,
                               "dominant_share_of_kernel_time": per_scan[dom] / sum(per_scan.values()),
                               "note": "isolated kernel time (scan's own iteration-0 scale/alpha) x GN iterations per "
                                       "scan; k_pko is latency-bound (sequential <=100-iteration EM), not HBM/MFMA-bound"},
        "multi_sequence": multi,
        "batched": batched,
        "pcie_inclusive": {"value": pcie_rate, "unit": "scans/s", "scans": n_pc,
                           "path": "lo_icp_optimize on host buffers (H2D points, D2H pose+logs, sync per scan)"},
        "roofline": {"kernel": corr_kernel, "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": traffic, "traffic_source": traffic_source, "traffic_live": traffic_live,
                     "alg_bytes_per_launch": alg_bytes, "points_per_launch": int(n0), "valid_fraction": v,
                     "timing": "isolated: back-to-back launches of the largest scan (lo_bench_kernel, HIP events)",
                     "kernel_us": kern_us[stage0],
                     "in_step": {"kernel_us": in_us.value, "scans": in_cnt.value,
                                 "achieved": (in_bytes / max(in_cnt.value, 1)) / (in_us.value * 1e-6) / 1e9 if in_us.value else None,
                                 "frac": (in_bytes / max(in_cnt.value, 1)) / (in_us.value * 1e-6) / 1e9 / HBM_PEAK_GBS
                                 if in_us.value else None,
                                 "timing": "each scan's first correspondence launch inside the GN loop (HIP events)"},
                     "working_set_bytes": ws_bytes, "in_cache": ws_bytes <= MALL_BYTES,
                     "in_cache_note": "working set (points + slot writes + one 32-B table sector per point) within the "
                                      "256 MB Infinity Cache: the fraction measures cache, not HBM, bandwidth"},
        "roofline_dominant": pko_roofline(em_live),
        "other_mode": other_mode,
    })
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(wl, args.cpu_budget, {args.mode: gpu_res, other: gpu_other}, args.mode)
        result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
    if rank == 0 and world == 1 and args.config == "kitti" and args.c5 > 0 and over_budget(args):
        result["c5_hbm"] = {"skipped": f"the run was past --full-budget ({args.full_budget:.0f} s) before this leg"}
    elif rank == 0 and world == 1 and args.config == "kitti" and args.c5 > 0:
        result["c5_hbm"] =c5_hbm_leg(local, dev, args.c5, pmc=args.pmc == "live", mode=args.mode)
    icp.close()
    if rank == 0:
        emit(result)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
