"""KITTI LiDAR frames on the device: KittiFileData and KittiDataset of the reference (dataset/kitti_dataset.py).

The reference crops a raw Velodyne frame to a box around the origin with Open3D, sorts it by x, takes ONE sample of
num_points_per_sample points of the whole cropped frame and centres it -- all in numpy, per frame, before the network sees
anything.  Here the frame is uploaded once and stays resident: pn2_frame_crop (box crop as an ordered compaction), pn2_scene_ingest
(the stable x-sort with its permutation) and pn2_frame_sample (fixed-size sample + centring), csrc/pn2_frame.hip and pn2_store.hip.

    frame = KittiFileData(points, box_size_x, box_size_y)             # points (n,3|4) float32: numpy array or device tensor
    centered, raw = frame.get_batch_of_one_z_box_from_origin(8192)    # (1,N,3) float32, (1,N,3) float64 on the device
    dataset = KittiDataset(8192, kitti_root, ["2011_09_26"], ["0095"], 60, 20)
    for frame in dataset.list_file_data: ...                          # a frame is read and uploaded when it is asked for

The crop keeps a row iff lo <= p <= hi on every axis, compared in float64, inclusive on both sides: the project's definition of
Open3D's crop_point_cloud.  Tie rule of the sort: rows with equal x stay in frame order (stable), where the
reference's np.argsort leaves the order among ties unspecified -- as SemanticDataset(ingest="device") documents for its scenes.
"""
import os

import numpy as np
import torch

from .._lib import launch, ptr, workspace

# KittiFileData.__init__ :15-16 of the reference: the z range of the region of interest
MIN_Z, MAX_Z = -2, 5
LABELS_NAMES = ["unlabeled", "man-made terrain", "natural terrain", "high vegetation", "low vegetation", "buildings", "hard scape",
                "scanning artifact", "cars"]
_INGEST_RES = 12  # int64 words pn2_scene_ingest reports into: z range (2), label histogram (9), status (1)


class KittiFileData:
    def __init__(self, points, box_size_x, box_size_y, device="cuda", seed=0):
        """points: (n,3) or (n,4) float32 (a KITTI row is x, y, z, intensity), a numpy array or a device tensor.  Crops to
        x, y in +-box_size/2 and z in [-2, 5] (kitti_dataset.py:15-26), then sorts by x (:35-38).  Afterwards: .points (cnt,3)
        float64 on the device, x-sorted; .labels (cnt,) int32 and .colors (cnt,3) float64 zeros; .source_index (cnt,) int32, an
        extension: the frame row of each .points row, so dense labels can be scattered back to the raw frame.

        The cropped count is read back once (it sizes every dense output and pn2_scene_ingest takes it as a host integer): the
        only host read on the per-frame path; get_batch_of_one_z_box_from_origin and the predictor add none.
        A frame with no point in the box raises ValueError (the reference would fail inside np.min)."""
        self.box_size_x, self.box_size_y = box_size_x, box_size_y
        self.seed = int(seed)
        self.file_path_without_ext = None
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("KittiFileData runs on the MI355X only: got device %s" % dev)
        if torch.is_tensor(points) and points.is_cuda:
            dev = points.device
        elif dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not torch.is_tensor(points):
            points = torch.from_numpy(np.ascontiguousarray(points))
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] not in (3, 4):
            raise ValueError("points: (n,3) or (n,4) float32, got %s %s" % (tuple(points.shape), points.dtype))
        n = int(points.shape[0])
        if n == 0:
            raise ValueError("no point of the frame lies in the box")
        frame = points.to(dev)
        if frame.stride(1) != 1 or frame.stride(0) < 3:  # rows read where they lie: (n,3) of an (n,4) frame keeps its stride of 4
            frame = frame.contiguous()
        with torch.cuda.device(dev):
            cropped = torch.empty((n, 3), dtype=torch.float64, device=dev)
            src = torch.empty((n,), dtype=torch.int32, device=dev)
            count = torch.empty((1,), dtype=torch.int32, device=dev)
            ws = workspace("pn2_frame_crop_workspace_size", dev, n)
            launch("pn2_frame_crop", dev, n, ptr(frame), int(frame.stride(0)), -box_size_x / 2.0, -box_size_y / 2.0, float(MIN_Z),
                   box_size_x / 2.0, box_size_y / 2.0, float(MAX_Z), ptr(cropped), ptr(src), ptr(count), ptr(ws), ws.numel())
            cnt = int(count.item())  # the one host read of the frame
            if cnt == 0:
                raise ValueError("no point of the frame lies in the box")
            self.points = torch.empty((cnt, 3), dtype=torch.float64, device=dev)
            perm = torch.empty((cnt,), dtype=torch.int32, device=dev)
            labels_u8 = torch.empty((cnt,), dtype=torch.uint8, device=dev)
            res = torch.empty((_INGEST_RES,), dtype=torch.int64, device=dev)
            ws = workspace("pn2_scene_ingest_workspace_size", dev, cnt)
            # (its status flags non-finite coordinates and labels: the crop has dropped the first, there are none of the second)
            launch("pn2_scene_ingest", dev, cnt, ptr(cropped), None, None, ptr(self.points), None, ptr(labels_u8), ptr(perm),
                   ptr(res[0:2]), ptr(res[2:11]), ptr(res[11:12]), ptr(ws), ws.numel())
            self.source_index = src[:cnt][perm.long()]
            self.labels = torch.zeros((cnt,), dtype=torch.int32, device=dev)
            self.colors = torch.zeros((cnt, 3), dtype=torch.float64, device=dev)
            self._counter = torch.zeros((1,), dtype=torch.int64, device=dev)
            self._sample_ws = workspace("pn2_frame_sample_workspace_size", dev, cnt)
        self.num_frame_points = n
        self.last_status = self.last_sel = None

    def __len__(self):
        return self.points.shape[0]

    def get_batch_of_one_z_box_from_origin(self, num_points_per_sample, sample_mask=None):
        """kitti_dataset.py:40-54: one sample of num_points_per_sample points of the whole cropped frame
        (_get_fix_sized_sample_mask: a frame of at most that many points is repeated, a larger one is subsampled) and its
        centring (_center_box, by the minimum of the SAMPLED points).
        sample_mask (cnt,) bool / uint8: the reference's shuffled boolean mask, replayed (used when cnt > N).  Default: a uniform
        random N-subset drawn on the device from (seed, a device counter that every call advances).
        -> centered (1,N,3) float32, raw (1,N,3) float64 on the device.  No host synchronisation: a rejected sample (a mask that
        does not select N points) comes back zero-filled and check_last() reports it."""
        dev, cnt, npts = self.points.device, len(self), int(num_points_per_sample)
        if npts <= 0:
            raise ValueError("num_points_per_sample must be positive")
        mask = None
        if sample_mask is not None:
            if not torch.is_tensor(sample_mask):
                sample_mask = torch.from_numpy(np.ascontiguousarray(np.asarray(sample_mask)).astype(np.uint8))
            if tuple(sample_mask.shape) != (cnt,):
                raise ValueError("sample_mask must be (%d,), one entry per cropped point" % cnt)
            mask = sample_mask.to(dev).to(torch.uint8).contiguous()
        with torch.cuda.device(dev):
            sel = torch.empty((npts,), dtype=torch.int32, device=dev)
            centered = torch.empty((1, npts, 3), dtype=torch.float32, device=dev)
            raw = torch.empty((1, npts, 3), dtype=torch.float64, device=dev)
            status = torch.empty((1,), dtype=torch.int32, device=dev)
            launch("pn2_frame_sample", dev, cnt, npts, ptr(self.points), ptr(mask), float(self.box_size_x), float(self.box_size_y),
                   self.seed, ptr(self._counter), ptr(self._sample_ws), self._sample_ws.numel(), ptr(sel), ptr(centered), ptr(raw),
                   ptr(status))
        self.last_status, self.last_sel = status, sel
        return centered, raw

    def check_last(self):
        """raise if the last sample was rejected (one host synchronisation)"""
        st = int(self.last_status.item())
        if st:
            raise RuntimeError("frame sampler status %d (3 mask does not select num_points_per_sample, 4 candidate list full)" % st)


def list_frames(base_dir, dates, drives):
    """the frames pykitti.raw(base_dir, date, drive).velo yields, in its order: per date and drive the files
    <base_dir>/<date>/<date>_drive_<drive>_sync/velodyne_points/data/*.bin sorted by name
    -> [(path, file_path_without_ext)], the name being "<date>/<drive>/%04d" % frame index within the drive (:102-104)"""
    frames = []
    for date in dates:
        for drive in drives:
            folder = os.path.join(base_dir, date, "%s_drive_%s_sync" % (date, drive), "velodyne_points", "data")
            names = sorted(f for f in os.listdir(folder) if f.endswith(".bin"))
            frames += [(os.path.join(folder, f), os.path.join(date, drive, "%04d" % k)) for k, f in enumerate(names)]
    return frames


class _FrameList:
    """dataset.list_file_data: len, indexing and iteration over the frames; each access reads the file and builds its
    KittiFileData (the reference holds every frame of a drive in memory: hundreds of frames of about 2 MB)"""

    def __init__(self, dataset):
        self._ds = dataset

    def __len__(self):
        return len(self._ds.frames)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._ds.load(k) for k in range(*i.indices(len(self)))]
        return self._ds.load(range(len(self))[i])

    def __iter__(self):
        return (self._ds.load(k) for k in range(len(self)))


class KittiDataset:
    def __init__(self, num_points_per_sample, base_dir, dates, drives, box_size_x, box_size_y, device="cuda", seed=0):
        """kitti_dataset.py:57-106.  Listing the drives touches no device; frame k is read (through one reusable pinned buffer)
        and uploaded by list_file_data[k], with the sampler seed `seed + k`."""
        self.num_points_per_sample = num_points_per_sample
        self.num_classes = 9
        self.labels_names = list(LABELS_NAMES)
        self.box_size_x, self.box_size_y = box_size_x, box_size_y
        self.device, self.seed = device, int(seed)
        self.frames = list_frames(base_dir, dates, drives)
        self.list_file_data = _FrameList(self)
        self._pinned = None
        self._copied = None  # the upload out of the pinned buffer has finished

    def get_file_paths_without_ext(self):
        return [name for _, name in self.frames]

    def read_frame(self, k):
        """frame k -> (n,4) float32 device tensor: x, y, z, intensity"""
        path = self.frames[k][0]
        nbytes = os.path.getsize(path)
        if nbytes % 16:
            raise ValueError("%s: %d bytes is not a whole number of float32 rows of 4" % (path, nbytes))
        dev = torch.device(self.device)
        if self._copied is not None:
            self._copied.synchronize()  # the host is about to overwrite the pinned buffer
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty((max(nbytes, 1 << 21),), dtype=torch.uint8).pin_memory()
        view, got = memoryview(self._pinned.numpy())[:nbytes], 0
        with open(path, "rb") as f:
            while got < nbytes:
                step = f.readinto(view[got:])
                if not step:
                    raise ValueError("%s: truncated" % path)
                got += step
        frame = self._pinned[:nbytes].view(torch.float32).reshape(-1, 4).to(dev, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(frame.device))
        return frame

    def load(self, k):
        file_data = KittiFileData(self.read_frame(k), self.box_size_x, self.box_size_y, device=self.device, seed=self.seed + k)
        file_data.file_path_without_ext = self.frames[k][1]
        return file_data
