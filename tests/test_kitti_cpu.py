"""CPU tests of the KITTI frame flow: the numpy model tests/frame_ref.py against the fixture frozen from the reference's own
code (tests/golden/kitti_frames.npz, made by tests/golden/make_kitti_golden.py), its tie rule, and the directory listing and
frame naming of pn2.dataset.KittiDataset (listing touches no device)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_ref as F  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "kitti_frames.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _case(gold, ci):
    tag = "c%d_" % ci
    n, cnt, bx, by, seed = (int(v) for v in gold[tag + "meta"])
    return dict(n=n, cnt=cnt, bx=bx, by=by, **{k: gold[tag + k] for k in ("frame", "source_index", "mask", "sel", "centered", "raw")})


def test_fixture_covers_the_cases(gold):
    assert int(gold["num_cases"]) == 8
    seen = set()
    for ci in range(8):
        c = _case(gold, ci)
        assert c["frame"].dtype == np.float32 and c["frame"].shape[1] == 4
        assert c["centered"].dtype == np.float64 and c["centered"].shape == (1, c["n"], 3) and c["raw"].shape == (1, c["n"], 3)
        assert len(c["mask"]) == (c["cnt"] if c["cnt"] > c["n"] else 0)
        rel = "below" if c["cnt"] < c["n"] else "equal" if c["cnt"] == c["n"] else "plus1" if c["cnt"] == c["n"] + 1 else "many"
        assert rel != "many" or c["cnt"] >= 4 * c["n"]
        seen.add((c["n"], rel))
    assert seen == {(n, r) for n in (16, 1024) for r in ("below", "equal", "plus1", "many")}
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("ci", range(8))
def test_model_reproduces_the_fixture(gold, ci):
    c = _case(gold, ci)
    pts, src = F.file_data(c["frame"], c["bx"], c["by"])
    assert len(pts) == c["cnt"] and np.array_equal(src, c["source_index"])
    assert np.array_equal(c["frame"][src, :3].astype(np.float64).view(np.int64), pts.view(np.int64))
    assert np.all(np.diff(pts[:, 0]) > 0)  # distinct x: np.argsort and the stable rule agree on these frames
    sel, cen, raw, status = F.sample(pts, c["n"], c["bx"], c["by"], mask=c["mask"] if c["cnt"] > c["n"] else None)
    assert status == F.ST_OK and np.array_equal(sel, c["sel"])
    assert np.array_equal(raw.view(np.int64), c["raw"][0].view(np.int64))
    assert np.array_equal(cen.view(np.int32), c["centered"][0].astype(np.float32).view(np.int32))
    # _center_box: the sample's minimum lands on (-bx/2, -by/2, 0) up to the float64 rounding of one subtraction
    assert np.allclose(c["centered"][0].min(axis=0), [-c["bx"] / 2, -c["by"] / 2, 0], atol=1e-12)


def test_ties_keep_frame_order():
    frame = F.tie_frame()
    pts, src = F.file_data(frame, 10, 10)
    p, s = F.crop(frame, *F.kitti_box(10, 10))
    order = np.argsort(p[:, 0], kind="stable")
    assert np.array_equal(src, s[order]) and np.array_equal(pts.view(np.int64), p[order].view(np.int64))
    same = pts[1:, 0] == pts[:-1, 0]
    assert same.sum() > 100 and np.all(src[1:][same] > src[:-1][same])  # within a run of equal x: ascending frame rows


def test_crop_is_inclusive_and_drops_non_finite():
    lo, hi = F.kitti_box(10, 10)
    rows = [[-5, 0, 0], [5, 0, 0], [0, -5, 0], [0, 5, 0], [0, 0, -2], [0, 0, 5]]
    frame = np.array(rows, dtype=np.float32)  # a value exactly on each of the six bounds: kept
    out = frame.copy()                        # the next float32 beyond each: dropped
    for k in range(6):
        a = k // 2
        out[k, a] = np.nextafter(frame[k, a], np.float32(np.inf if frame[k, a] > 0 else -np.inf))
    bad = np.zeros((9, 3), dtype=np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            bad[3 * k + a, a] = v
    p, src = F.crop(np.concatenate([frame, out, bad, np.array([[-0.0, -0.0, -0.0]], dtype=np.float32)]), lo, hi)
    assert list(src) == [0, 1, 2, 3, 4, 5, 21] and np.signbit(p[-1]).all()


def test_select_device_mode_is_the_n_smallest_keys():
    from dataset_stream_ref import draw64, sample_stream
    sel, status = F.select(500, 64, seed=3, counter=2)
    keys = draw64(sample_stream(3, 2, 0), np.arange(500, dtype=np.uint64))
    assert status == 0 and len(sel) == 64 and np.all(np.diff(sel) > 0)
    assert keys[sel].max() < np.delete(keys, sel).min()
    assert not np.array_equal(sel, F.select(500, 64, seed=3, counter=3)[0])
    assert F.select(100, 16, mask=np.r_[np.ones(15), np.zeros(85)])[1] == F.ST_MASK


def _write_layout(root, date, drive, names):
    folder = os.path.join(root, date, "%s_drive_%s_sync" % (date, drive), "velodyne_points", "data")
    os.makedirs(folder)
    for k, name in enumerate(names):
        np.full((3 + k, 4), k, dtype=np.float32).tofile(os.path.join(folder, name))
    return folder


def test_listing_and_frame_names(pn2, tmp_path):
    root = str(tmp_path)
    a = _write_layout(root, "2011_09_26", "0095", ["0000000002.bin", "0000000000.bin", "0000000001.bin", "notes.txt"])
    b = _write_layout(root, "2011_09_26", "0001", ["0000000005.bin", "0000000007.bin"])
    frames = pn2.dataset.kitti_dataset.list_frames(root, ["2011_09_26"], ["0095", "0001"])
    assert [p for p, _ in frames] == [os.path.join(a, "000000000%d.bin" % k) for k in range(3)] + [
        os.path.join(b, "0000000005.bin"), os.path.join(b, "0000000007.bin")]
    # the reference names a frame by its position within the drive, not by its file name
    assert [n for _, n in frames] == [os.path.join("2011_09_26", "0095", "%04d" % k) for k in range(3)] + [
        os.path.join("2011_09_26", "0001", "0000"), os.path.join("2011_09_26", "0001", "0001")]
    ds = pn2.dataset.KittiDataset(8192, root, ["2011_09_26"], ["0095", "0001"], 60, 20)  # listing only: no device is touched
    assert ds.num_classes == 9 and len(ds.labels_names) == 9 and ds.labels_names[0] == "unlabeled" and ds.labels_names[8] == "cars"
    assert len(ds.list_file_data) == 5 and ds.get_file_paths_without_ext() == [n for _, n in frames]
    assert pn2.dataset.KittiDataset is pn2.dataset.kitti_dataset.KittiDataset
    assert pn2.dataset.KittiFileData is pn2.dataset.kitti_dataset.KittiFileData


def test_no_color_hyperparams_are_the_reference_settings(pn2):
    hp, base = pn2.model.SEMANTIC_NO_COLOR_HYPERPARAMS, pn2.model.SEMANTIC_HYPERPARAMS
    assert hp["use_color"] == 0 and (hp["box_size_x"], hp["box_size_y"]) == (60, 20)
    assert {k: v for k, v in hp.items() if k not in ("use_color", "box_size_x", "box_size_y")} == \
        {k: v for k, v in base.items() if k != "use_color"}


def test_entry_points_refuse_bad_arguments(pn2):
    """argument validation comes before any launch (placeholder pointers are never dereferenced)"""
    L, nul, p = pn2._lib.lib, None, 256
    assert "pn2_frame_sample" in pn2._lib._STATEFUL and "pn2_frame_crop" not in pn2._lib._STATEFUL
    box = (-5.0, -5.0, -2.0, 5.0, 5.0, 5.0)
    assert L.pn2_frame_crop(0, p, 4, *box, p, p, p, p, 1 << 20, nul) == -1
    assert L.pn2_frame_crop(10, p, 2, *box, p, p, p, p, 1 << 20, nul) == -1
    assert L.pn2_frame_crop(10, nul, 4, *box, p, p, p, p, 1 << 20, nul) == -2
    assert L.pn2_frame_crop(10, p, 4, *box, p, p, nul, p, 1 << 20, nul) == -2
    assert L.pn2_frame_crop(10, p, 4, *box, p, p, p, p, 0, nul) == -1          # workspace too small
    assert L.pn2_frame_crop(10, p, 4, *box, p, p, p, p + 4, 1 << 20, nul) == -1  # workspace misaligned
    assert L.pn2_frame_crop((1 << 24) + 1, p, 4, *box, p, p, p, p, 1 << 20, nul) == -3
    need = pn2._lib.u64_array([0])
    assert L.pn2_frame_crop_workspace_size(1025, need) == 0 and need[0] == 256 and L.pn2_frame_crop_workspace_size(0, need) == -1
    assert L.pn2_frame_sample_workspace_size(100, need) == 0 and need[0] % 256 == 0 and need[0] > 4096 * 16
    ws = int(need[0])
    assert L.pn2_frame_sample(0, 16, p, nul, 10.0, 10.0, 0, p, p, ws, p, p, p, p, nul) == -1
    assert L.pn2_frame_sample(100, 16, p, nul, 0.0, 10.0, 0, p, p, ws, p, p, p, p, nul) == -1
    assert L.pn2_frame_sample(100, 16, p, nul, 10.0, 10.0, 0, nul, p, ws, p, p, p, p, nul) == -2  # device mode needs the counter
    assert L.pn2_frame_sample(100, 16, nul, p, 10.0, 10.0, 0, nul, p, ws, p, p, p, p, nul) == -2
    assert L.pn2_frame_sample(100, 16, p, p, 10.0, 10.0, 0, nul, p, ws - 1, p, p, p, p, nul) == -1
