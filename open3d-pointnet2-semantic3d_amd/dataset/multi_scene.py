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

ingest="device" builds the store where it will lie instead (csrc/pn2_store.hip: sort by x, gather, z range and label
histogram per scene in one call): the constructor then needs the GPU, and the per-scene arrays are views of the store.
"""
import json
import os

import numpy as np
import torch

from .._lib import launch, ptr, u64_array
from ..util.metric import SEMANTIC3D_LABELS_NAMES
from ..util.point_cloud_util import load_labels, read_point_cloud, scene_path

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


def label_weights_from_counts(counts_per_scene):
    """the second half of label_weights_of: per scene the nine counts of np.histogram(labels, range(10)) (the host path takes
    them from numpy, the device path from pn2_scene_ingest) -> summed in float64, cast to float32, normalised -> float32 (9,)"""
    w = np.zeros(9)
    for tmp in counts_per_scene:
        w += tmp
    w = w.astype(np.float32)
    w = w / np.sum(w)
    return 1 / np.log(1.2 + w)


def label_weights_of(labels_per_scene):
    """1 / log(1.2 + class frequency) over the scenes (semantic_dataset.py:280-290): np.histogram over range(10) (its last
    bin is closed: labels 8 and 9 share it), summed in float64, cast to float32, normalised -> float32 (9,)."""
    return label_weights_from_counts(np.histogram(labels, range(10))[0] for labels in labels_per_scene)


_INGEST_RES = 12  # int64 words per scene that pn2_scene_ingest's small outputs share: zrange (2 float64), hist (9), status


def _ingest_labels(labels, dev):
    """labels of any integer or bool dtype, a tensor or an array -> int32 on dev.  A dtype wider than int32 is clamped to
    [-1, 256] first: what lies outside [0, 255] stays outside, and nothing wraps into it."""
    if not torch.is_tensor(labels):
        labels = np.asarray(labels)
        if labels.dtype.kind not in "iub":
            raise ValueError("labels: an integer or bool dtype, got %s" % labels.dtype)
        if labels.dtype.kind != "b" and labels.dtype.itemsize >= 4 and labels.dtype != np.int32:
            labels = np.minimum(labels, 256) if labels.dtype.kind == "u" else np.clip(labels, -1, 256)
        return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    if labels.dtype.is_floating_point or labels.dtype.is_complex:
        raise ValueError("labels: an integer or bool dtype, got %s" % labels.dtype)
    labels = labels.to(dev)
    if labels.dtype not in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32):
        labels = labels.to(torch.int64).clamp(-1, 256)  # (an unsigned value that wraps lands on -1: still outside)
    return labels.to(torch.int32).contiguous()


def _rank_seed(seed):
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        seed = int(seed) ^ (torch.distributed.get_rank() * 0x9E3779B97F4A7C15)
    return int(seed) & 0xFFFFFFFFFFFFFFFF


class SemanticDataset:
    def __init__(self, num_points_per_sample, split, use_color, box_size_x, box_size_y, path, device="cuda", seed=0,
                 scenes=None, splits=None, ingest="host", keep_perm=False):
        """The reference's constructor (semantic_dataset.py:214-290).  path/split: loads <path>/<name>.pcd and .labels for
        every scene name of the split (test: no labels).  scenes=[(points, labels, colors, name), ...]: the arrays
        directly (labels / colors may be None).  splits: overrides the split -> scene-name table.
        ingest="host": the scenes are read, sorted by x and measured in numpy; scene_points / scene_labels / scene_colors are
        host arrays and the store is uploaded by the first sample call.
        ingest="device": the store is built in HBM by pn2_scene_ingest (csrc/pn2_store.hip), one call per scene, straight into
        the scene's slice: files are read by scene_io.read_point_cloud / preprocess.load_labels, `scenes` may hold device
        tensors (points float32 / float64, labels of any integer or bool dtype, colours float) or host arrays (uploaded once);
        nothing of a scene's size comes back to the host.  scene_points / scene_labels / scene_colors are then device views of
        the store (float64, uint8, float32; scene_colors[i] is None without colour).  Rows with equal x keep their input order
        (a stable sort; numpy's default argsort on the host path leaves that order unspecified), so the two stores are equal
        bit for bit wherever a scene's x values are distinct.  A NaN or an infinity in a coordinate is a ValueError.
        keep_perm (ingest="device"): scene_perm[i], an int32 device tensor, maps a position in the sorted scene to its row in the
        input (last_sel - scene_offsets[scene] indexes it)."""
        if ingest not in ("host", "device"):
            raise ValueError("ingest: 'host' or 'device', got %r" % (ingest,))
        if keep_perm and ingest != "device":
            raise ValueError("keep_perm needs ingest='device'")
        self.ingest = ingest
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
            if ingest == "device":  # read scene by scene, straight into the store
                scenes = [(None, None, None, name) for name in table[split]]
            else:
                scenes = []
                for name in table[split]:
                    prefix = os.path.join(path, name)
                    pts, cols = read_point_cloud(scene_path(prefix))  # <scene>.pcd, else <scene>.ply
                    labels = load_labels(prefix + ".labels") if has_label else None
                    scenes.append((pts, labels, cols, name))
        if not scenes:
            raise ValueError("no scenes")
        self.scene_names, self.file_paths_without_ext = [], []
        self.scene_points, self.scene_labels, self.scene_colors = [], [], []
        self._store = None
        if ingest == "device":
            counts, z_size, hists = self._ingest_device(scenes, has_label, keep_perm)
        else:
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
            counts = [len(p) for p in self.scene_points]
            # scene_z_size of _extract_z_box (:132), once per scene
            z_size = [np.max(p, axis=0)[2] - np.min(p, axis=0)[2] for p in self.scene_points]
        self.num_scenes = len(counts)
        self.scene_counts = np.array(counts, dtype=np.int64)
        total = self.get_total_num_points()
        if total >= 2 ** 31:
            raise ValueError("the store holds at most 2^31 - 1 points")
        self.scene_probas = np.array([c / total for c in counts], dtype=np.float64)  # :268-271
        cdf = self.scene_probas.cumsum()  # np.random.choice(..., p=scene_probas)
        self.scene_cdf = cdf / cdf[-1]
        self.scene_offsets = np.concatenate([[0], np.cumsum(self.scene_counts)]).astype(np.int64)
        self.scene_z_size = np.array(z_size)
        if split not in ("train", "train_full"):
            self.label_weights = np.zeros(9)
        elif ingest == "device":
            self.label_weights = label_weights_from_counts(hists)
        else:
            self.label_weights = label_weights_of(self.scene_labels)
        if ingest == "host":  # (pn2_scene_ingest's status said the same of the device store)
            for lab in self.scene_labels:
                if lab.size and (lab.min() < 0 or lab.max() > 255):
                    raise ValueError("labels must lie in [0, 255]")
        self.max_chunks = int(max(1, max((c + _CHUNK - 1) // _CHUNK for c in self.scene_counts)))
        self._dev = None

    # ---- ingest="device" ---------------------------------------------------------------------------------------------
    def _ingest_device(self, scenes, has_label, keep_perm):
        """Builds the resident store (self._store: points (total,3) float64, colors (total,3) float32 or None, labels (total,)
        uint8) with one pn2_scene_ingest call per scene, each writing its scene's slice, and sets the per-scene attributes to
        views of it.  scenes: (points, labels, colors, name) with tensors or arrays, or (None, None, None, name) for a scene
        read from <path>/<name>.pcd and .labels.  One workspace, sized for the largest scene, serves every call; per scene one
        96-byte read-back (z range, label histogram, status).  -> counts [n], scene_z_size (ns,) float64, hists (ns,9) int64"""
        from .. import preprocess, scene_io  # (they import this package's siblings: not at module level)
        from ..util.point_cloud_util import read_pcd_layout, read_ply_header
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("ingest='device' builds the store on the MI355X: got device %s (there is no CPU path in the "
                             "product; ingest='host' keeps the scenes in numpy)" % dev)
        if dev.index is None:
            dev = self.device = torch.device("cuda", torch.cuda.current_device())
        counts = []
        for pts, _, _, name in scenes:
            if pts is None:
                file_path = scene_path(os.path.join(self.path, name))
                with open(file_path, "rb") as f:
                    n = read_ply_header(f).n if file_path.endswith(".ply") else read_pcd_layout(f).n
            else:
                n = int(np.prod(tuple(pts.shape))) // 3 if hasattr(pts, "shape") else len(np.asarray(pts).reshape(-1, 3))
            if n == 0:
                raise ValueError("scene %r has no points" % (name,))
            counts.append(n)
        total = sum(counts)
        if total >= 2 ** 31:
            raise ValueError("the store holds at most 2^31 - 1 points")
        ws_bytes, nbytes = 0, u64_array([0])
        for n in sorted(set(counts)):  # (a host-side query; the sort's share need not grow with n)
            launch("pn2_scene_ingest_workspace_size", dev, n, nbytes, stream=False)
            ws_bytes = max(ws_bytes, int(nbytes[0]))
        with torch.cuda.device(dev):
            store = dict(points=torch.empty((total, 3), dtype=torch.float64, device=dev),
                         colors=torch.empty((total, 3), dtype=torch.float32, device=dev) if self.use_color else None,
                         labels=torch.empty((total,), dtype=torch.uint8, device=dev))
            perm = torch.empty((total,), dtype=torch.int32, device=dev) if keep_perm else None
            ws = torch.empty((ws_bytes + 256,), dtype=torch.uint8, device=dev)
            ws = ws[(-ws.data_ptr()) % 256:]
            res = torch.empty((len(scenes), _INGEST_RES), dtype=torch.int64, device=dev)
        z_size, hists, o = [], [], 0
        if keep_perm:
            self.scene_perm = []
        for k, ((pts, labels, cols, name), n) in enumerate(zip(scenes, counts)):
            if pts is None:
                prefix = os.path.join(self.path, name)
                pts, cols = scene_io.read_point_cloud(scene_path(prefix), dev, want_colors=self.use_color)
                labels = preprocess.load_labels(prefix + ".labels", dev) if has_label else None
            if torch.is_tensor(pts):
                if not pts.dtype.is_floating_point:
                    raise ValueError("scene %r: points float32 or float64, got %s" % (name, pts.dtype))
                pts = pts.to(dev, torch.float64).reshape(-1, 3).contiguous()
            else:
                pts = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))).to(dev)
            labels = None if (labels is None or not has_label) else _ingest_labels(labels, dev)
            if cols is None or not self.use_color:
                cols = None
            elif torch.is_tensor(cols):
                cols = cols.to(dev, torch.float64).contiguous()
            else:
                cols = torch.from_numpy(np.ascontiguousarray(cols, dtype=np.float64)).to(dev)
            if pts.shape[0] != n or (labels is not None and tuple(labels.shape) != (n,)) or \
                    (cols is not None and tuple(cols.shape) != (n, 3)):
                raise ValueError("scene %r: labels (n,) and colors (n,3) must match points (n,3)" % (name,))
            e = o + n
            out_c = None if store["colors"] is None else store["colors"][o:e]
            if out_c is not None and cols is None:
                out_c.zero_()  # colour asked for, none given: zeros, as on the host path
            launch("pn2_scene_ingest", dev, n, ptr(pts), ptr(cols), ptr(labels), ptr(store["points"][o:e]), ptr(out_c),
                   ptr(store["labels"][o:e]), None if perm is None else ptr(perm[o:e]), ptr(res[k, 0:2]), ptr(res[k, 2:11]),
                   ptr(res[k, 11:12]), ptr(ws), ws.numel())
            r = res[k].cpu()  # the scene's one read-back; the inputs above may go once it has returned
            status = int(r[11:12].view(torch.int32)[0])
            if status == 1:
                raise ValueError("scene %r: non-finite coordinate" % (name,))
            if status == 2:
                raise ValueError("labels must lie in [0, 255]")
            zr = r[0:2].view(torch.float64).numpy()
            z_size.append(zr[1] - zr[0])
            hists.append(r[2:11].numpy().copy())
            self.scene_points.append(store["points"][o:e])
            self.scene_labels.append(store["labels"][o:e])
            self.scene_colors.append(out_c)
            if keep_perm:
                self.scene_perm.append(perm[o:e])
            self.scene_names.append(name)
            self.file_paths_without_ext.append(os.path.join(self.path, name) if self.path else name)
            o = e
        self._store = store
        return counts, np.array(z_size), np.array(hists, dtype=np.int64).reshape(-1, 9)

    # ---- the reference's small methods -------------------------------------------------------------------------------
    def get_total_num_points(self):
        return np.sum(self.scene_counts)

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
            if self._store is not None:  # ingest="device": the store already lies in HBM
                big = self._store
            else:
                big = dict(points=t(np.concatenate(self.scene_points), np.float64),
                           colors=t(np.concatenate(self.scene_colors), np.float32) if self.use_color else None,
                           labels=t(np.concatenate(self.scene_labels).astype(np.uint8), np.uint8))
            d = dict(points=big["points"], colors=big["colors"], labels=big["labels"],
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

    def tile_cover(self, scene, phase=(0.0, 0.0), min_points=1):
        """The tiled cover of scene `scene` (pn2_tile_plan, csrc/pn2_tile.hip): the scene cut into box_size_x x box_size_y
        columns on a grid shifted by `phase` (metres, >= 0), every column with at least min_points points split into as many
        num_points_per_sample-sized samples as it takes to use each of its points once.  -> TileCover.  One plan call and one
        32-byte read-back (the header); works on ingest="host" (the store is uploaded first) and ingest="device" stores."""
        scene = int(scene)
        if not 0 <= scene < self.num_scenes:
            raise ValueError("scene %d: the store holds scenes 0 .. %d" % (scene, self.num_scenes - 1))
        px, py = float(phase[0]), float(phase[1])
        if not (0.0 <= px < float("inf") and 0.0 <= py < float("inf")):
            raise ValueError("phase: two finite offsets >= 0, got %r" % (phase,))
        if int(min_points) < 1:
            raise ValueError("min_points must be at least 1")
        v = self._scene_view(self._upload(1), scene)
        return TileCover(self, scene, v["points"], v["colors"], (px, py), int(min_points))

    def check_last(self):
        """raise if a sample of the last batch was rejected (zero-filled); one host synchronisation."""
        st = self.last_status.cpu().tolist()
        if any(st):
            raise RuntimeError("SemanticDataset: rejected samples: %s" % {i: STATUS_NAMES.get(v, v) for i, v in enumerate(st) if v})



TILE_STATUS_NAMES = {1: "non-finite x or y", 2: "tile index outside [0, 2^31)", 3: "more samples than the table holds"}


class TileCover:
    """One pass of the tiled cover of a scene (SemanticDataset.tile_cover): `order` (n,) int32, `samples` (num_samples,4) int32
    rows [a, m, s, S] and `header` (8,) int32 on the device, as pn2_tile_plan leaves them (include/pn2_abi.h has the rule), and
    from the header's one read-back num_tiles, num_samples and skipped_points.  Sample q holds num_points_per_sample rows of
    one column; its first live[q] rows are the one occurrence of their points in this pass, the rest repeat them."""

    def __init__(self, dataset, scene, points, colors, phase, min_points):
        dev = dataset.device
        n, npts = int(points.shape[0]), dataset.num_points_per_sample
        self.scene, self.phase, self.min_points, self.num_points = scene, phase, min_points, n
        self.num_points_per_sample = npts
        self.box_size_x, self.box_size_y = float(dataset.box_size_x), float(dataset.box_size_y)
        self.use_color = dataset.use_color
        self._points, self._colors, self._dev = points, colors if dataset.use_color else None, dev
        nbytes = u64_array([0])
        launch("pn2_tile_plan_workspace_size", dev, n, nbytes, stream=False)
        with torch.cuda.device(dev):
            ws = torch.empty((int(nbytes[0]) + 256,), dtype=torch.uint8, device=dev)
            ws = ws[(-ws.data_ptr()) % 256:]
            self.order = torch.empty((n,), dtype=torch.int32, device=dev)
            self.header = torch.empty((8,), dtype=torch.int32, device=dev)
            # every sample holds at least one point of its own: n rows hold any table (cut to num_samples rows below)
            table = torch.empty((n, 4), dtype=torch.int32, device=dev)
        launch("pn2_tile_plan", dev, n, ptr(points), self.box_size_x, self.box_size_y, phase[0], phase[1], npts, min_points, n,
               ptr(self.order), ptr(table), ptr(self.header), ptr(ws), ws.numel())
        h = self.header.cpu().tolist()  # the one host read of the pass
        if h[3] != 0:
            raise ValueError("scene %r: %s" % (dataset.scene_names[scene], TILE_STATUS_NAMES.get(h[3], h[3])))
        self.num_tiles, self.num_samples, self.skipped_points = h[0], h[1], h[2]
        self.samples = table[:max(self.num_samples, 1)].clone()  # (one row at least: a pointer for an empty table)

    def batch(self, q0, batch_size):
        """-> data (B,N,6|3) float32 (centred xyz [| rgb]), sel (B,N) int32 (positions in the x-sorted scene), live (B,) int32
        for samples q0 .. q0 + B - 1 (pn2_tile_gather).  A slot beyond the last sample repeats it with live = 0 (every batch
        has the full shape); a cover without samples gives zeros, sel = -1, live = 0.  No host synchronisation."""
        b, npts, dev = int(batch_size), self.num_points_per_sample, self._dev
        if b <= 0 or int(q0) < 0:
            raise ValueError("batch_size must be positive and q0 non-negative")
        data = torch.empty((b, npts, 6 if self.use_color else 3), dtype=torch.float32, device=dev)
        sel = torch.empty((b, npts), dtype=torch.int32, device=dev)
        live = torch.empty((b,), dtype=torch.int32, device=dev)
        launch("pn2_tile_gather", dev, b, npts, int(q0), int(self.use_color), ptr(self._points), ptr(self._colors),
               ptr(self.order), ptr(self.samples), ptr(self.header), self.box_size_x, self.box_size_y, ptr(data), ptr(sel),
               ptr(live))
        return data, sel, live
