"""What aligning two LiDAR frames costs ("Rigid registration"): one JSON line with, per estimator, in this one
process, after a warm-up call of the same shape:
  icp_ms    pn2_icp alone between two device events on the caller's stream -- the workspace and the outputs allocated before
            the first event, nothing read by the host in between --, the median of --rounds timings; the same with
            max_iteration = 0 (the grid and one evaluation: what evaluate_registration costs), so that
            per_round_ms = (icp_ms - evaluate_ms) / max_iteration is one match + step pair, the early-out launches included;
  call_ms   pn2.registration_icp end to end on a host clock, the device synchronised on both sides (allocation, the one host
            read); point-to-plane includes no normals: they are estimated once, outside;
  host      an ICP on the host with the same correspondence distance, stop criterion and initial pose: scipy.spatial.cKDTree
            for the partners and numpy's SVD (Kabsch) for the point-to-point step, one timing; its pose is compared with the
            device's.  Without scipy the baseline is brute force in numpy on a subsample of 4000 x 4000 points, and the line
            says so.
The case: the synthetic 120 000-point LiDAR-like frame of tools/cluster_cost.py as the target and the same frame, subsampled to
every other point and moved by 1.5 degrees and 0.3 m, as the source, at a correspondence distance of 0.5 m.
usage: python tools/icp_cost.py [--rounds 7] [--max_iteration 30] [--no-host]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pn2_amd as pn2  # noqa: E402
from cluster_cost import frame, wall_ms  # noqa: E402

MAX_DISTANCE = 0.5
NORMAL_RADIUS = 0.8


def motion():
    t = np.radians(1.5)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    T[:3, 3] = [0.25, -0.15, 0.05]
    return T


def clouds():
    """-> source (60 000,3), target (120 000,3) float32, truth: source -> target"""
    target, _ = frame()
    truth = motion()
    inv = np.linalg.inv(truth)
    source = (target[::2].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return source, target, truth


def device_ms(lib, dev, src, tgt, nrm, est, max_iteration, rounds):
    """pn2_icp between device events -> the timings in ms, and the (result, header) buffer of the last call"""
    ns, nt = len(src), len(tgt)
    corr = torch.empty((ns,), dtype=torch.int32, device=dev)
    out = torch.zeros((24,), dtype=torch.float64, device=dev)
    nbytes = ctypes.c_ulonglong(0)
    lib.launch("pn2_icp_workspace_size", dev, ns, nt, max_iteration, ctypes.byref(nbytes), stream=False)
    ws = torch.empty((int(nbytes.value) + 255,), dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    times = []
    for _ in range(rounds + 1):  # the first is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lib.launch("pn2_icp", dev, ns, lib.ptr(src), None, nt, lib.ptr(tgt), None, lib.ptr(nrm), MAX_DISTANCE, est, None, max_iteration,
                   1e-6, 1e-6, lib.ptr(corr), lib.ptr(out), None, lib.ptr(out, 160), ws.data_ptr() + off, ws.numel() - off)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times[1:], out.cpu().numpy()


def host_icp(source, target, max_iteration):
    """point-to-point on the host -> seconds, T, iterations, what it is"""
    s, t = source.astype(np.float64), target.astype(np.float64)
    try:
        from scipy.spatial import cKDTree
        what = "cKDTree + numpy Kabsch, all points"
    except ImportError:
        cKDTree = None
        rs = np.random.RandomState(0)
        s, t = s[rs.choice(len(s), 4000, replace=False)], t[rs.choice(len(t), 4000, replace=False)]
        what = "no scipy: brute force + numpy Kabsch on a subsample of 4000 x 4000 points"
    t0 = time.perf_counter()
    tree = cKDTree(t) if cKDTree else None
    T = np.eye(4)
    prev = None
    k = 0
    while True:
        moved = s @ T[:3, :3].T + T[:3, 3]
        if tree is not None:
            dist, at = tree.query(moved, distance_upper_bound=MAX_DISTANCE)
            has = np.isfinite(dist)
        else:
            d2 = ((moved[:, None, :] - t[None, :, :]) ** 2).sum(2)
            at = d2.argmin(1)
            dist = np.sqrt(d2[np.arange(len(s)), at])
            has = dist <= MAX_DISTANCE
        fitness, rmse = has.mean(), np.sqrt((dist[has] ** 2).mean()) if has.any() else 0.0
        if (prev is not None and abs(fitness - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6) or k == max_iteration or has.sum() < 3:
            return time.perf_counter() - t0, T, k, what
        p, u = moved[has], t[at[has]]
        pc, uc = p.mean(0), u.mean(0)
        U, _, Vt = np.linalg.svd((u - uc).T @ (p - pc))
        Rm = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = Rm, uc - Rm @ pc
        T, prev, k = step @ T, (fitness, rmse), k + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max_iteration", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = pn2._lib
    source, target, truth = clouds()
    d_src, d_tgt = torch.from_numpy(source).to(dev), torch.from_numpy(target).to(dev)
    normals = pn2.estimate_normals(d_tgt, NORMAL_RADIUS, viewpoint=(0, 0, 0))
    out = {"source_points": len(source), "target_points": len(target), "max_distance": MAX_DISTANCE, "max_iteration": args.max_iteration,
           "device": torch.cuda.get_device_name(dev), "estimators": {}}
    for name, est in pn2.icp.ESTIMATIONS.items():
        nrm = normals if est else None
        full, buf = device_ms(lib, dev, d_src, d_tgt, nrm, est, args.max_iteration, args.rounds)
        ev, _ = device_ms(lib, dev, d_src, d_tgt, nrm, est, 0, args.rounds)
        header = buf[20:].view(np.int32)

        def call():
            return pn2.registration_icp(d_src, d_tgt, MAX_DISTANCE, estimation=name, target_normals=nrm, max_iteration=args.max_iteration)

        call()
        runs = [wall_ms(call) for _ in range(args.rounds)]
        angle, dist = pn2.icp.rigid_error(buf[:16].reshape(4, 4), truth)
        out["estimators"][name] = {
            "icp_ms": {"median": round(float(np.median(full)), 3), "runs": [round(v, 3) for v in full]},
            "evaluate_ms": {"median": round(float(np.median(ev)), 3), "runs": [round(v, 3) for v in ev]},
            "per_round_ms": round(float(np.median(full) - np.median(ev)) / max(1, args.max_iteration), 4),
            "call_ms": {"median": round(float(np.median(runs)), 3), "runs": [round(v, 3) for v in runs]},
            "status": int(header[0]), "pairs": int(header[3]), "updates": int(header[4]), "converged": int(header[5]),
            "fitness": round(float(buf[16]), 4), "rmse": round(float(buf[17]), 5),
            "pose_error_deg": round(angle, 5), "pose_error_m": round(dist, 5)}
    if not args.no_host:
        seconds, T, k, what = host_icp(source, target, args.max_iteration)
        angle, dist = pn2.icp.rigid_error(T, truth)
        out["host"] = {"what": what, "seconds": round(seconds, 3), "updates": k, "pose_error_deg": round(angle, 5),
                       "pose_error_m": round(dist, 5),
                       "over_icp": round(seconds * 1e3 / out["estimators"]["point_to_point"]["icp_ms"]["median"], 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
