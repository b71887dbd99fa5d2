"""Pins tests/multiscene_ref.py to the REFERENCE's own multi-scene sampler and freezes the result (run where the reference
checkout exists):

    python tests/golden/make_multiscene_golden.py      -> tests/golden/multiscene_sampler.npz

dataset/semantic_dataset.py and util/provider.py cannot be imported (open3d, tensorflow-era imports), so SemanticDataset
(__init__, sample_batch_in_all_files, sample_in_all_files, ...), SemanticFileData's sampling methods and
rotate_feature_point_cloud / rotate_point_cloud are lifted out of the reference's source files with `ast` -- unmodified,
never copied into this repository -- and executed with stand-ins for the Open3D file loading.  np.random is seen through a
thin recording wrapper, so every draw is stored and the device sampler can replay it.  The restatement must reproduce the
lifted reference bit for bit under the same stream."""
import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_DS = "/root/reference/dataset/semantic_dataset.py"
REF_PROV = "/root/reference/util/provider.py"

import multiscene_ref as R  # noqa: E402


def lift(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), (path, names)
    exec(compile(ast.fix_missing_locations(ast.Module(body=keep, type_ignores=[])), path, "exec"), ns)
    return ns


class RecordingNumpy(types.ModuleType):
    """`np` for the lifted code: numpy itself, except np.random, which is the recorder"""

    def __init__(self, rec):
        super().__init__("np")
        self.random = rec

    def __getattr__(self, k):
        return getattr(np, k)


def lifted_reference(scenes, splits, rec):
    npx = RecordingNumpy(rec)
    prov = types.SimpleNamespace(**lift(REF_PROV, ["rotate_point_cloud", "rotate_feature_point_cloud"], {"np": npx}))
    ns = lift(REF_DS, ["SemanticFileData", "SemanticDataset"], {"np": npx, "os": os, "provider": prov,
                                                                "map_name_to_file_prefixes": splits, "print": lambda *a: None})
    FileData = ns["SemanticFileData"]
    by_name = {name: (p, l, c) for p, l, c, name in scenes}

    def stand_in_init(self, file_path_without_ext, has_label, use_color, box_size_x, box_size_y):
        # what open3d.read_point_cloud + load_labels give the reference's __init__ (:60-88): float64 arrays, then x-sorted
        self.file_path_without_ext = file_path_without_ext
        self.box_size_x, self.box_size_y = box_size_x, box_size_y
        p, l, c = by_name[os.path.basename(file_path_without_ext)]
        self.points = p.copy()
        self.labels = l.copy() if has_label else np.zeros(len(p)).astype(bool)
        self.colors = c.copy() if use_color else np.zeros_like(p)
        sort_idx = np.argsort(self.points[:, 0])
        self.points, self.labels, self.colors = self.points[sort_idx], self.labels[sort_idx], self.colors[sort_idx]

    FileData.__init__ = stand_in_init
    return ns["SemanticDataset"]


# (split, use_color, augment, batch, npts, box, seed)
CASES = [("train", True, True, 8, 256, 4, 0), ("train", False, True, 8, 256, 4, 1),
         ("validation", True, False, 8, 256, 4, 2), ("train", True, False, 8, 256, 4, 3),
         ("validation", False, False, 6, 128, 6, 4)]


def main():
    import pn2_amd as pn2
    scenes = R.synthetic_scenes()
    splits = {"train": [s[3] for s in scenes], "validation": [s[3] for s in scenes[1:]]}
    out = {}
    for ci, (split, use_color, augment, b, n, box, seed) in enumerate(CASES):
        rec = R.Recorder()
        Ref = lifted_reference(scenes, splits, rec)
        ref = Ref(n, split, use_color, box, box, "data")
        np.random.seed(seed)
        data, lab, wts = ref.sample_batch_in_all_files(b, augment=augment)
        draws = rec.draws(b)
        # the restatement, on the same stream and the package's host attributes
        ds = pn2.dataset.SemanticDataset(n, split, use_color, box, box, "data", device="cpu",
                                         scenes=[s for s in scenes if s[3] in splits[split]])
        assert np.array_equal(ds.scene_probas, np.array(ref.scene_probas))
        assert ds.label_weights.dtype == np.asarray(ref.label_weights).dtype
        assert np.array_equal(ds.label_weights, ref.label_weights)
        np.random.seed(seed)
        mine = R.sample_batch(R.HostDataset(ds), b, augment, R.Recorder())
        for a, m in zip((data, lab, wts), mine):
            assert a.dtype == m.dtype and np.array_equal(a, m), "restatement differs from the reference"
        cnt = [int(R.column(ds.scene_points[k], ds.scene_points[k][c], box / 2, box / 2).sum())
               for k, c in zip(draws["scene"], draws["center"])]
        tag = "c%d_" % ci
        out[tag + "meta"] = np.array([b, n, box, int(use_color), int(augment), seed])
        out[tag + "split"] = np.array(split)
        out[tag + "data"], out[tag + "label"], out[tag + "weights"] = data, lab.astype(np.int32), wts
        out[tag + "data_dtype"] = np.array(str(data.dtype))
        out[tag + "weights_dtype"] = np.array(str(wts.dtype))
        out[tag + "cnt"] = np.array(cnt)
        for k, v in draws.items():
            out[tag + "draw_" + k] = v
        out[tag + "scene_probas"] = np.array(ref.scene_probas)
        out[tag + "label_weights"] = np.asarray(ref.label_weights)
        out[tag + "total"] = np.array(ref.get_total_num_points())
        out[tag + "num_batches"] = np.array([ref.get_num_batches(k) for k in (1, 2, 4, 16)])
        print("case %d: %s color=%d augment=%d cnt=%s scenes=%s" % (ci, split, use_color, augment, cnt, draws["scene"]))
    out["splits_train"] = np.array(splits["train"])
    out["splits_validation"] = np.array(splits["validation"])
    path = os.path.join(ROOT, "tests", "golden", "multiscene_sampler.npz")
    np.savez_compressed(path, **out)
    print("restatement == lifted reference on %d cases; %s: %d bytes" % (len(CASES), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
