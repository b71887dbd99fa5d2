"""Device-resident multi-scene sampler: SemanticDataset of the reference (dataset/semantic_dataset.py:214-343, fed to
train.py:122-130) with every scene in one store in HBM.

The reference builds each training batch in numpy inside an mp.Pool: per sample it picks a scene with probability
proportional to its point count, crops a column around a random centre point, samples it to num_points_per_sample points,
looks up label_weights[labels] and, with augment=True, rotates the xyz about z by a random angle
(util/provider.py rotate_feature_point_cloud / rotate_point_cloud); the batch then crosses PCIe.  Here
`sample_batch_in_all_files` is one call of pn2_dataset_sample (csrc/pn2_dataset.hip: four launches, no host
synchronisation, no torch kernel) and returns the batch on the device in the layout Trainer.train_step / eval_step take:
data (B,N,6|3) float32, labels (B,N) int32, weights (B,N) float32, all contiguous.

Random numbers.  With draws=None every draw (scene, centre, subset keys, angle) is a counter-based hash of (seed, batch
counter, sample, index) made on the device; the batch counter lives in device memory and the last launch of a call advances
it, so a torch.cuda.graph capture of one call replays into fresh batches.  Under torch.distributed the rank is folded into
the seed (seed ^ rank * 0x9E3779B97F4A7C15): every rank draws its own stream of batches.  draws=dict(scene, center, masks,
angle) replays the reference's np.random draws instead (parity tests; costs host work).

The host-side attributes (scene_probas, label_weights, counts, the split table) need no GPU; the store is uploaded on the
first sample call.  Call it once eagerly before capturing it in a graph.  One call at a time per dataset object: the
workspace is shared between calls.
"""
import json
import os

import numpy as np
import torch

from .._lib import launch, ptr, u64_array
from ..util.metric import SEMANTIC3D_LABELS_NAMES
from ..util.point_cloud_util import load_labels, read_point_cloud_pcd

_SPLITS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "semantic3d_splits.json")
_CHUNK = 1024  # slab points per chunk in csrc/pn2_dataset.hip
_INFO = 8
STATUS_NAMES = {1: "empty column or bad draw", 2: "column wider than the masks", 3: "mask does not select N points",
                4: "candidate list full", 5: "slab longer than the store allows"}


def default_splits():
    """split -> scene names, from semantic3d_splits.json (train, validation, test and the unions train_full, all)."""
    with open(_SPLITS_JSON) as f:
        tab = json.load(f)
    out = {k: list(v) for k, v in tab["splits"].items()}
    for k, parts in tab["unions"].items():
        out[k] = [name for p in parts for name in tab["splits"][p]]
    return out


def label_weights_of(labels_per_scene):
    """1 / log(1.2 + class frequency) over the scenes (semantic_dataset.py:280-290): np.histogram over range(10) (its last
    bin is closed: labels 8 and 9 share it), summed in float64, cast to float32, normalised -> float32 (9,)."""
    w = np.zeros(9)
    for labels in labels_per_scene:
        tmp, _ = np.histogram(labels, range(10))
        w += tmp
    w = w.astype(np.float32)
    w = w / np.sum(w)
    return 1 / np.log(1.2 + w)


def _rank_seed(seed):
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        seed = int(seed) ^ (torch.distributed.get_rank() * 0x9E3779B97F4A7C15)
    return int(seed) & 0xFFFFFFFFFFFFFFFF


class SemanticDataset:
    def __init__(self, num_points_per_sample, split, use_color, box_size_x, box_size_y, path, device="cuda", seed=0,
                 scenes=None, splits=None):
        """The reference's constructor (semantic_dataset.py:214-290).  path/split: loads <path>/<name>.pcd and .labels for
        every scene name of the split (test: no labels).  scenes=[(points, labels, colors, name), ...]: the arrays
        directly (labels / colors may be None).  splits: overrides the split -> scene-name table."""
        self.num_points_per_sample = int(num_points_per_sample)
        self.split = split
        self.use_color = bool(use_color)
        self.box_size_x, self.box_size_y = box_size_x, box_size_y
        self.num_classes = 9
        self.path = path
        self.labels_names = list(SEMANTIC3D_LABELS_NAMES)
        self.device = torch.device(device)
        self.seed = _rank_seed(seed)
        has_label = split != "test"
        if self.num_points_per_sample <= 0 or not (box_size_x > 0 and box_size_y > 0):
            raise ValueError("num_points_per_sample and the box sizes must be positive")
        if scenes is None:
            table = splits if splits is not None else default_splits()
            if split not in table:
                raise ValueError("unknown split %r (known: %s)" % (split, sorted(table)))
            scenes = []
            for name in table[split]:
                prefix = os.path.join(path, name)
                pts, cols = read_point_cloud_pcd(prefix + ".pcd")
                labels = load_labels(prefix + ".labels") if has_label else None
                scenes.append((pts, labels, cols, name))
        if not scenes:
            raise ValueError("no scenes")
        self.scene_names, self.file_paths_without_ext = [], []
        self.scene_points, self.scene_labels, self.scene_colors = [], [], []
        for pts, labels, cols, name in scenes:
            pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
            if len(pts) == 0:
                raise ValueError("scene %r has no points" % (name,))
            labels = np.zeros(len(pts), dtype=bool) if (labels is None or not has_label) else np.asarray(labels)
            cols = np.asarray(cols, dtype=np.float64) if (cols is not None and self.use_color) else np.zeros_like(pts)
            if labels.shape != (len(pts),) or cols.shape != pts.shape:
                raise ValueError("scene %r: labels (n,) and colors (n,3) must match points (n,3)" % (name,))
            sort_idx = np.argsort(pts[:, 0])  # SemanticFileData.__init__ (:84-88)
            self.scene_points.append(np.ascontiguousarray(pts[sort_idx]))
            self.scene_labels.append(np.ascontiguousarray(labels[sort_idx]))
            self.scene_colors.append(np.ascontiguousarray(cols[sort_idx]))
            self.scene_names.append(name)
            self.file_paths_without_ext.append(os.path.join(path, name) if path else name)
        self.num_scenes = len(self.scene_points)
        self.scene_counts = np.array([len(p) for p in self.scene_points], dtype=np.int64)
        total = self.get_total_num_points()
        if total >= 2 ** 31:
            raise ValueError("the store holds at most 2^31 - 1 points")
        self.scene_probas = np.array([len(p) / total for p in self.scene_points], dtype=np.float64)  # :268-271
        cdf = self.scene_probas.cumsum()  # np.random.choice(..., p=scene_probas)
        self.scene_cdf = cdf / cdf[-1]
        self.scene_offsets = np.concatenate([[0], np.cumsum(self.scene_counts)]).astype(np.int64)
        # scene_z_size of _extract_z_box (:132), once per scene
        self.scene_z_size = np.array([np.max(p, axis=0)[2] - np.min(p, axis=0)[2] for p in self.scene_points])
        if split in ("train", "train_full"):
            self.label_weights = label_weights_of(self.scene_labels)
        else:
            self.label_weights = np.zeros(9)
        for lab in self.scene_labels:
            if lab.size and (lab.min() < 0 or lab.max() > 255):
                raise ValueError("labels must lie in [0, 255]")
        self.max_chunks = int(max(1, max((c + _CHUNK - 1) // _CHUNK for c in self.scene_counts)))
        self._dev = None

    # ---- the reference's small methods -------------------------------------------------------------------------------
    def get_total_num_points(self):
        return np.sum([len(p) for p in self.scene_points])

    def get_num_batches(self, batch_size):
        return int(self.get_total_num_points() / (batch_size * self.num_points_per_sample))

    def get_file_paths_without_ext(self):
        return list(self.file_paths_without_ext)

    # ---- device store ------------------------------------------------------------------------------------------------
    def _upload(self, batch_size):
        """the resident store (uploaded once) with `workspace` = the workspace of this batch size.  One workspace per batch
        size: pn2_dataset_sample lays its workspace out by b and keeps only the histogram and candidate counts of THAT layout
        zero between calls, so a workspace shared between batch sizes would hand a larger b the candidate lists of a smaller one
        where it expects zeros (samples rejected with "candidate list full")."""
        d = self._dev
        dev = self.device
        if d is None:
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
            d = dict(points=t(np.concatenate(self.scene_points), np.float64),
                     colors=t(np.concatenate(self.scene_colors), np.float32) if self.use_color else None,
                     labels=t(np.concatenate(self.scene_labels).astype(np.uint8), np.uint8),
                     offsets=t(self.scene_offsets, np.int32), cdf=t(self.scene_cdf, np.float64),
                     zsize=t(self.scene_z_size, np.float64), lw=t(self.label_weights, np.float32),
                     counter=torch.zeros(1, dtype=torch.int64, device=dev), workspaces={})
            self._dev = d
        ws = d["workspaces"].get(batch_size)
        if ws is None:
            nbytes = u64_array([0])  # written by the query
            launch("pn2_dataset_workspace_size", dev, batch_size, self.max_chunks, nbytes, stream=False)
            ws = torch.zeros(nbytes[0] + 256, dtype=torch.uint8, device=dev)  # kept zero by the kernels
            d["workspaces"][batch_size] = ws
        d["workspace"] = ws
        return d

    @property
    def batch_counter(self):
        """device int64 (1,): batches drawn so far from the device random numbers."""
        return self._upload(1)["counter"]

    def sample_batch_in_all_files(self, batch_size, augment=True, draws=None):
        """-> batch_data (B,N,6) float32 ([xyz | rgb]; (B,N,3) without colour), batch_label (B,N) int32, batch_weights
        (B,N) float32 (label_weights[label]), on the device.  draws=None: device random numbers; draws=dict(scene=(B,),
        center=(B,) (relative to its scene, as np.random.randint(0, len(points)) draws it), masks=(B,cap) uint8 (the
        reference's shuffled mask for columns wider than N), angle=(B,) float64 (np.random.uniform() * 2 * np.pi)): the
        reference's np.random draws, replayed.  Afterwards last_scene, last_center, last_cnt, last_sel (store indices:
        scene offset + position in the x-sorted scene) and last_angle describe the batch.
        augment=util.provider.Augmenter(...): the sampler runs with its own rotation off and the augmenter runs on its batch
        in the same stream (pn2_augment: two or three more launches; labels and weights follow a shuffle); the augmenter's
        last_* attributes say what it applied."""
        b, n = int(batch_size), self.num_points_per_sample
        augmenter = None
        if callable(augment):
            augmenter, augment = augment, False
        if b <= 0:
            raise ValueError("batch_size must be positive")
        d = self._upload(b)
        dev = self.device
        c = 6 if self.use_color else 3
        data = torch.empty((b, n, c), dtype=torch.float32, device=dev)
        label = torch.empty((b, n), dtype=torch.int32, device=dev)
        weights = torch.empty((b, n), dtype=torch.float32, device=dev)
        sel = torch.empty((b, n), dtype=torch.int32, device=dev)
        info = torch.empty((b, _INFO), dtype=torch.int32, device=dev)
        finfo = torch.empty((b, 3), dtype=torch.float64, device=dev)
        scene = center = mask = rot = None
        cap = 0
        if draws is not None:
            scene_h = np.asarray(draws["scene"]).astype(np.int64).reshape(-1)
            center_h = np.asarray(draws["center"]).astype(np.int64).reshape(-1)
            if scene_h.shape != (b,) or center_h.shape != (b,):
                raise ValueError("draws['scene'] and draws['center'] must hold batch_size entries")
            if scene_h.min() < 0 or scene_h.max() >= self.num_scenes:
                raise ValueError("draws['scene'] out of range")
            if np.any(center_h < 0) or np.any(center_h >= self.scene_counts[scene_h]):
                raise ValueError("draws['center'] out of range of its scene")
            scene = torch.from_numpy(scene_h.astype(np.int32)).to(dev)
            center = torch.from_numpy(center_h.astype(np.int32)).to(dev)
            m = draws.get("masks")
            if m is not None:
                mask = torch.as_tensor(np.asarray(m)).to(dev).to(torch.uint8).contiguous()
                if mask.dim() != 2 or mask.shape[0] != b:
                    raise ValueError("draws['masks'] must be (batch_size, capacity)")
                cap = int(mask.shape[1])
            if augment:
                ang = np.asarray(draws["angle"], dtype=np.float64).reshape(-1)
                if ang.shape != (b,):
                    raise ValueError("draws['angle'] must hold batch_size entries")
                rot = torch.from_numpy(np.stack([ang, np.cos(ang), np.sin(ang)], 1)).to(dev)
        ws = d["workspace"]
        base = (-ws.data_ptr()) % 256
        launch("pn2_dataset_sample", dev,
               b, n, self.num_scenes, self.max_chunks, int(self.use_color), int(bool(augment)), ptr(d["points"]),
               ptr(d["colors"]), ptr(d["labels"]), ptr(d["offsets"]), ptr(d["cdf"]), ptr(d["zsize"]), ptr(d["lw"]),
               int(d["lw"].numel()), self.box_size_x / 2, self.box_size_y / 2, self.seed, ptr(d["counter"]), ptr(scene),
               ptr(center), ptr(mask), cap, ptr(rot), ptr(ws[base:]), ws.numel() - base, ptr(info), ptr(finfo), ptr(sel),
               ptr(data), ptr(label), ptr(weights))
        self.last_scene, self.last_center, self.last_cnt = info[:, 0], info[:, 1], info[:, 2]
        self.last_status, self.last_sel, self.last_angle = info[:, 7], sel, finfo[:, 0]
        if augmenter is not None:  # in place unless it shuffles
            return augmenter(data, label, weights, out=None if augmenter.shuffle else data)
        return data, label, weights

    def _scene_view(self, d, scene):
        """the one-scene view of the store pn2_dataset_sample reads for `scene`: its slices of points / colours / labels and its
        small tables (offsets [0, count], cdf [1.0], its scene_z_size), made once per scene and kept on the device"""
        views = d.setdefault("views", {})
        v = views.get(scene)
        if v is None:
            dev = self.device
            o, e = int(self.scene_offsets[scene]), int(self.scene_offsets[scene + 1])
            v = dict(offset=o, points=d["points"][o:e], colors=None if d["colors"] is None else d["colors"][o:e],
                     labels=d["labels"][o:e], offsets=torch.tensor([0, e - o], dtype=torch.int32).to(dev),
                     cdf=torch.ones(1, dtype=torch.float64).to(dev),
                     zsize=torch.tensor([self.scene_z_size[scene]], dtype=torch.float64).to(dev),
                     max_chunks=int(max(1, (e - o + _CHUNK - 1) // _CHUNK)))
            views[scene] = v
        return v

    def sample_batch_in_file(self, scene, batch_size):
        """The reference's list_file_data[scene].sample_batch(batch_size, num_points_per_sample) (semantic_dataset.py:57-82, as
        predict.py:163 calls it) on the resident store: every sample is a column of scene `scene`, un-augmented, drawn from
        the device random numbers.  -> data (B,N,6|3) float32 (centred xyz [| rgb]), points_raw (B,N,3) float64 (the same
        points as they lie in the scene), labels (B,N) int32, on the device.  pn2_dataset_sample on a one-scene view of the
        store: no (B, len(scene)) tensor, no host synchronisation.  Advances batch_counter like any other batch; afterwards
        last_scene (= scene), last_center, last_cnt, last_sel (store indices) and last_status describe the batch."""
        b, n = int(batch_size), self.num_points_per_sample
        if b <= 0:
            raise ValueError("batch_size must be positive")
        scene = int(scene)
        if not 0 <= scene < self.num_scenes:
            raise ValueError("scene %d: the store holds scenes 0 .. %d" % (scene, self.num_scenes - 1))
        d = self._upload(b)
        v = self._scene_view(d, scene)
        dev = self.device
        data = torch.empty((b, n, 6 if self.use_color else 3), dtype=torch.float32, device=dev)
        label = torch.empty((b, n), dtype=torch.int32, device=dev)
        weights = torch.empty((b, n), dtype=torch.float32, device=dev)
        sel = torch.empty((b, n), dtype=torch.int32, device=dev)
        info = torch.empty((b, _INFO), dtype=torch.int32, device=dev)
        finfo = torch.empty((b, 3), dtype=torch.float64, device=dev)
        ws = d["workspace"]  # this batch size's own, sized for the store's longest scene: enough for any one of them
        base = (-ws.data_ptr()) % 256
        launch("pn2_dataset_sample", dev,
               b, n, 1, v["max_chunks"], int(self.use_color), 0, ptr(v["points"]), ptr(v["colors"]), ptr(v["labels"]),
               ptr(v["offsets"]), ptr(v["cdf"]), ptr(v["zsize"]), None, 0, self.box_size_x / 2, self.box_size_y / 2, self.seed,
               ptr(d["counter"]), None, None, None, 0, None, ptr(ws[base:]), ws.numel() - base, ptr(info), ptr(finfo), ptr(sel),
               ptr(data), ptr(label), ptr(weights))
        # view-local -> store indices; a rejected sample keeps its -1 (its rows of points_raw are then the store's last point:
        # check_last() tells)
        self.last_sel = torch.where(sel < 0, sel, sel + v["offset"])
        points_raw = d["points"][self.last_sel.long()]
        self.last_scene = torch.full((b,), scene, dtype=torch.int32, device=dev)
        self.last_center, self.last_cnt = info[:, 1], info[:, 2]
        self.last_status, self.last_angle = info[:, 7], finfo[:, 0]
        return data, points_raw, label

    def check_last(self):
        """raise if a sample of the last batch was rejected (zero-filled); one host synchronisation."""
        st = self.last_status.cpu().tolist()
        if any(st):
            raise RuntimeError("SemanticDataset: rejected samples: %s" % {i: STATUS_NAMES.get(v, v) for i, v in enumerate(st) if v})

