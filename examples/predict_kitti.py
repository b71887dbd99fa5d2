"""Labels for the frames of a KITTI raw drive on one MI355X: the __main__ of the reference's kitti_predict.py without its visualiser.

    python examples/predict_kitti.py --kitti_root <dir> [--ckpt file] [--save]
    python examples/predict_kitti.py --synthetic 3 120000 [--save]     # no dataset: F frames of N points in the KITTI layout

Per frame: read the .bin, crop / sort / sample / centre on the device (pn2.dataset.KittiDataset), colourless forward + argmax and
the 3-NN vote onto the whole cropped frame (pn2.kitti_predict.PredictInterpolator), and with --save the dense cloud and its labels
as result/dense/<frame>.pcd and .labels (pn2.scene_io), then the reference's timer line.  Each phase ends with a device
synchronisation so that its time is its own, as the reference's session.run calls do.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

DATE, DRIVE = "2011_09_26", "0095"  # kitti_predict.py:136-138


def synthetic_frame(rs, n):
    """(n,4) float32 rows x, y, z, intensity: ground around z = -1.7 (the sensor sits that high), returns out to 80 m, denser near
    the sensor as a spinning LiDAR's are"""
    r = 80.0 * rs.random_sample(n) ** 2
    a = rs.uniform(0, 2 * np.pi, n)
    z = -1.7 + np.abs(rs.normal(0, 1.0, n)) * (rs.random_sample(n) < 0.4)
    return np.stack([r * np.cos(a), r * np.sin(a), z, rs.random_sample(n)], 1).astype(np.float32)


def write_synthetic_drive(root, frames, n, seed=0):
    folder = os.path.join(root, DATE, "%s_drive_%s_sync" % (DATE, DRIVE), "velodyne_points", "data")
    os.makedirs(folder, exist_ok=True)
    rs = np.random.RandomState(seed)
    for k in range(frames):
        synthetic_frame(rs, n).tofile(os.path.join(folder, "%010d.bin" % k))


def run(flags, kitti_root):
    hyper_params = dict(pn2.model.SEMANTIC_NO_COLOR_HYPERPARAMS)
    dense_output_dir = os.path.join("result", "dense")
    if flags.save:
        os.makedirs(dense_output_dir, exist_ok=True)
    dataset = pn2.dataset.KittiDataset(num_points_per_sample=hyper_params["num_point"], base_dir=kitti_root, dates=[DATE],
                                       drives=[DRIVE], box_size_x=hyper_params["box_size_x"],
                                       box_size_y=hyper_params["box_size_y"])
    predictor = pn2.kitti_predict.PredictInterpolator(flags.ckpt or None, dataset.num_classes, hyper_params)
    print("Model restored" if flags.ckpt else "Fresh variables (no --ckpt)")
    for k in range(len(dataset.list_file_data)):
        timer = {"load_data": 0, "predict_interpolate": 0, "write_data": 0, "total": 0}
        global_start_time = time.time()

        start_time = time.time()
        kitti_file_data = dataset.list_file_data[k]
        points_centered, points = kitti_file_data.get_batch_of_one_z_box_from_origin(hyper_params["num_point"])
        torch.cuda.synchronize()
        timer["load_data"] += time.time() - start_time

        start_time = time.time()
        dense_points = kitti_file_data.points
        dense_labels, dense_colors = predictor.predict_and_interpolate(points_centered, points, dense_points)
        torch.cuda.synchronize()
        timer["predict_interpolate"] += time.time() - start_time

        if flags.save:
            start_time = time.time()
            file_prefix = os.path.basename(kitti_file_data.file_path_without_ext)
            dense_pcd_path = os.path.join(dense_output_dir, file_prefix + ".pcd")
            pn2.scene_io.write_point_cloud_pcd(dense_pcd_path, dense_points)
            print("Exported dense_pcd to {}".format(dense_pcd_path))
            dense_labels_path = os.path.join(dense_output_dir, file_prefix + ".labels")
            pn2.scene_io.write_labels(dense_labels_path, dense_labels)
            print("Exported dense_labels to {}".format(dense_labels_path))
            timer["write_data"] += time.time() - start_time

        timer["total"] += time.time() - global_start_time
        fmt_string = "[{:5.2f} FPS] " + ": {:.04f}, ".join(timer.keys()) + ": {:.04f}"
        print(fmt_string.format(*([1.0 / timer["total"]] + list(timer.values()))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--ckpt", default="", help="Checkpoint file (train.Trainer.save); none: fresh variables")
    parser.add_argument("--save", action="store_true", default=False)
    parser.add_argument("--kitti_root", default="", help="KITTI raw root; with --synthetic: where the frames are written")
    parser.add_argument("--synthetic", type=int, nargs=2, metavar=("F", "N"), help="write F frames of N points and run on them")
    flags = parser.parse_args()
    if not flags.synthetic:
        if not flags.kitti_root:
            parser.error("--kitti_root or --synthetic is required")
        return run(flags, flags.kitti_root)
    if flags.kitti_root:
        write_synthetic_drive(flags.kitti_root, *flags.synthetic)
        return run(flags, flags.kitti_root)
    with tempfile.TemporaryDirectory() as root:
        write_synthetic_drive(root, *flags.synthetic)
        run(flags, root)


if __name__ == "__main__":
    main()
