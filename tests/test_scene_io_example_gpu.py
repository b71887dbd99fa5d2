"""examples/predict_semantic3d.py on its --data / --raw route: the dense clouds come through pn2.read_point_cloud_pcd and
pn2.load_labels as device tensors, the results leave through the device writers.  The input files are written with the host
writers and the outputs read with the host readers, so neither side of the check runs the code under test."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N, C = 2048, 9


@pytest.mark.timeout(300)
def test_example_data_route_reads_and_writes_on_the_device(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    spec = importlib.util.spec_from_file_location("predict_semantic3d_example", os.path.join(ROOT, "examples", "predict_semantic3d.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    with open(os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "dataset", "semantic3d_splits.json")) as f:
        import json
        names = json.load(f)["splits"]["validation"]
    data, raw = tmp_path / "data", tmp_path / "raw"
    data.mkdir()
    raw.mkdir()
    scene_points, samples, dense = 30000, 3, {}
    for k, name in enumerate(names):
        pts, labels, colors = example.synthetic_scene(300 + k, scene_points, 30.0, 20.0)
        if k % 2:
            labels = None  # a scene without dense ground truth
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(cuda, dt)  # noqa: E731
        sp, sc, sl = pn2.downsample.down_sample_arrays(t(pts, torch.float64), t(colors, torch.float64),
                                                       t(np.clip((pts[:, 2] / 0.7).astype(np.int32) + 1, 1, 8), torch.int32), voxel_size=0.1)
        U.write_point_cloud_pcd(str(data / (name + ".pcd")), sp.cpu().numpy(), sc.cpu().numpy())
        U.write_labels(str(data / (name + ".labels")), sl.cpu().numpy())
        U.write_point_cloud_pcd(str(raw / (name + ".pcd")), pts, colors)
        if labels is not None:
            U.write_labels(str(raw / (name + ".labels")), labels)
        dense[name] = labels
    cmd = [sys.executable, os.path.join(ROOT, "examples", "predict_semantic3d.py"), "--data", str(data), "--raw", str(raw), "--num_samples",
           str(samples), "--batch-size", "2", "--points", str(N), "--npoint", "256,64,32,16", "--chunk", "12500"]
    run = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-3000:]
    with_truth = sum(v is not None for v in dense.values())
    assert "Sparse results" in out and "Global results" in out and out.count("Confusion matrix:") == with_truth + 2
    for name in names:
        sparse_dir, dense_dir = tmp_path / "result" / "sparse", tmp_path / "result" / "dense"
        sp, _ = U.read_point_cloud_pcd(str(sparse_dir / (name + ".pcd")))
        sl = U.load_labels(str(sparse_dir / (name + ".labels")))
        assert sp.shape == (samples * N, 3) and sl.shape == (samples * N,) and sl.min() >= 0 and sl.max() < C
        want_p, _ = U.read_point_cloud_pcd(str(raw / (name + ".pcd")))
        dp, dc = U.read_point_cloud_pcd(str(dense_dir / (name + "_colored.pcd")))
        dl = U.load_labels(str(dense_dir / (name + ".labels")))
        assert dp.tobytes() == want_p.tobytes() and dl.shape == (scene_points,)  # the dense cloud went through the device reader
        lab, col = pn2.predict.label_dense(sp.astype(np.float32), sl, dp.astype(np.float32))
        assert np.array_equal(lab.cpu().numpy(), dl)
        assert np.array_equal(col.cpu().numpy(), np.rint(dc * 255.0).astype(np.uint8))
