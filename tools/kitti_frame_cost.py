"""What one KITTI frame costs ("KITTI frames"): one JSON line, on a synthetic 120 000-point frame with rows of
4 (a real Velodyne frame is about that size), the 10 x 10 box and N = 8192, medians of 7 runs after a warm-up:
  1 device_prepare_ms  : upload of the raw frame, pn2_frame_crop, the x-sort, pn2_frame_sample, with the one count read
                         (KittiFileData + get_batch_of_one_z_box_from_origin);
  2 host_prepare_ms    : the same steps in numpy on the host (crop, argsort, shuffled mask, centring) plus the upload of the batch
                         and of the cropped frame the dense vote needs -- the only way without the frame kernels;
  3 predict_ms         : PredictInterpolator.predict_and_interpolate (graph replay + 3-NN vote onto the cropped frame);
  4 frames_per_s       : the whole frame, 1 + 3.
usage: python tools/kitti_frame_cost.py [--points 120000] [--num-point 8192]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import pn2_amd as pn2  # noqa: E402
import predict_kitti as ex  # noqa: E402

BOX = 10


def wall_ms(fn, reps=7):
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(v)), 3), [round(x, 3) for x in v]


def host_prepare(frame, n, dev):
    """kitti_dataset.py:15-54 in numpy (the crop as the inclusive rule), then the uploads"""
    p = frame[:, :3].astype(np.float64)
    lo, hi = np.array([-BOX / 2, -BOX / 2, -2.0]), np.array([BOX / 2, BOX / 2, 5.0])
    p = p[np.all((p >= lo) & (p <= hi), axis=1)]
    p = p[np.argsort(p[:, 0])]
    if len(p) > n:
        mask = np.concatenate((np.ones(n, dtype=bool), np.zeros(len(p) - n, dtype=bool)))
        np.random.shuffle(mask)
    else:
        mask = np.arange(n) % len(p)
    s = p[mask]
    box_min = s.min(axis=0)
    centered = (s - np.array([box_min[0] + BOX / 2, box_min[1] + BOX / 2, box_min[2]])).astype(np.float32)
    return (torch.from_numpy(centered[None]).to(dev), torch.from_numpy(s[None]).to(dev), torch.from_numpy(p).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--num-point", type=int, default=8192)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.num_point
    hp = dict(pn2.model.SEMANTIC_NO_COLOR_HYPERPARAMS, num_point=n, box_size_x=BOX, box_size_y=BOX)
    frame = ex.synthetic_frame(np.random.RandomState(0), args.points)
    pinned = torch.from_numpy(frame).pin_memory()
    out = {"frame_points": args.points, "num_point": n, "box": BOX}

    def device_prepare():
        fd = pn2.dataset.KittiFileData(pinned.to(dev, non_blocking=True), BOX, BOX, device=dev)
        return fd, fd.get_batch_of_one_z_box_from_origin(n)

    fd, (centered, raw) = device_prepare()  # warm-up: library, allocator
    fd.check_last()
    out["cropped_points"] = len(fd)
    predictor = pn2.kitti_predict.PredictInterpolator(None, 9, hp, device=dev)
    predictor.predict_and_interpolate(centered, raw, fd.points)  # captures
    host_prepare(frame, n, dev)

    def whole():
        f, (c, r) = device_prepare()
        return predictor.predict_and_interpolate(c, r, f.points)

    out["device_prepare_ms"], out["device_prepare_runs"] = wall_ms(device_prepare)
    out["host_prepare_ms"], out["host_prepare_runs"] = wall_ms(lambda: host_prepare(frame, n, dev))
    out["predict_ms"], out["predict_runs"] = wall_ms(lambda: predictor.predict_and_interpolate(centered, raw, fd.points))
    out["frame_ms"], out["frame_runs"] = wall_ms(whole)
    out["frames_per_s"] = round(1e3 / out["frame_ms"], 1)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
