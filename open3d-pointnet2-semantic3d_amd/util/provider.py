"""Point-cloud augmentation on the device: the reference's util/provider.py as calls of pn2_augment (csrc/pn2_augment.hip).

The reference augments a batch in numpy on the host.  Here every function takes and returns device float32 tensors (B,N,C)
with xyz in channels 0:3, makes ONE pn2_augment call with one stage on, and keeps the reference's name, signature and
defaults; `Augmenter` runs any set of stages as one fused call.  The contract -- stage order (shuffle, rotation, scale,
shift, jitter, dropout), the float64-between-stages arithmetic rule, how every draw is formed -- is written once, in
include/pn2_abi.h.

Random numbers.  With draws=None every draw is a counter-based hash of (seed, batch counter, cloud, index) made on the device;
the batch counter is a device int64 that each call advances, so a torch.cuda.graph capture of a call replays into fresh
draws.  The module-level functions share one counter per device, seeded by `seed()`.  draws=dict(...) replays numpy's draws
instead and reproduces the reference's functions bit for bit (parity tests; costs host work):
    perm (N,)            shuffle_points: the shuffled np.arange(N)
    angle (B,)           rotate_*: np.random.uniform() * 2 * np.pi per cloud
    normals (B,3)        rotate_perturbation_*: np.random.randn(3) per cloud
    matrix (B,3,3)       Augmenter only: the rotation matrices themselves (instead of angle / normals)
    scale (B,)  shift (B,3)  noise (B,N,C or 3) standard normals  ratio (B,) (already times max_dropout_ratio)  u (B,N)

Where this differs from the reference, on purpose: scale and shift act on xyz only and a channel no stage touches is copied
(the reference scales every channel and zero-fills the channels its rotate_* functions do not name); jitter_point_cloud
returns float32 (the float32 cast of the reference's float64 result).  Like the reference, shift_point_cloud,
random_scale_point_cloud, random_point_dropout and rotate_point_cloud_with_normal work in place and return their argument.
getDataFiles and load_h5 (HDF5 file lists) are not part of this module.
"""
import numpy as np
import torch

from .._lib import ABI, launch, ptr, require_cuda, u64_array

_K = ABI.constants
SHUFFLE, ROTATE, PERTURB, SCALE, SHIFT, JITTER, DROPOUT, ROTATE_NORMALS, JITTER_ALL, REPLAY = (
    _K["PN2_AUG_" + k] for k in ("SHUFFLE", "ROTATE", "PERTURB", "SCALE", "SHIFT", "JITTER", "DROPOUT", "ROTATE_NORMALS",
                                 "JITTER_ALL", "REPLAY"))
_PARAMS = _K["PN2_AUG_PARAMS"]
_AXES = {"x": 0, "y": 1, "z": 2}


# ---- host side of the replay mode: the matrices as numpy builds them ---------------------------------------------------
def axis_matrix(axis, angle):
    """the reference's matrix of a rotation by `angle` about "x" | "y" | "z" (points are ROW vectors: p @ R), float64"""
    c, s = np.cos(angle), np.sin(angle)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, s], [0, -s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    if axis == "z":
        return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
    raise ValueError("Wrong rotation axis")


def perturbation_matrix(normals, angle_sigma, angle_clip):
    """Rz . (Ry . Rx) of the three angles clip(angle_sigma * normals, -angle_clip, angle_clip), float64"""
    a = np.clip(angle_sigma * np.asarray(normals, dtype=np.float64), -angle_clip, angle_clip)
    rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    return np.dot(rz, np.dot(ry, rx))


def _matrices(b, axis, perturb, draws):
    """(B,3,3) float64 of a replayed call: draws['matrix'], or R_axis . R_perturb from draws['angle'] / draws['normals']"""
    if "matrix" in draws:
        m = np.asarray(draws["matrix"], dtype=np.float64)
    else:
        m = np.empty((b, 3, 3))
        for k in range(b):
            r = None
            if axis is not None:
                r = axis_matrix(axis, np.asarray(draws["angle"], dtype=np.float64).reshape(-1)[k])
            if perturb is not None:
                rp = perturbation_matrix(np.asarray(draws["normals"]).reshape(-1, 3)[k], *perturb)
                r = rp if r is None else np.dot(r, rp)
            m[k] = r
    if m.shape != (b, 3, 3):
        raise ValueError("the rotation draws must give one (3,3) matrix per cloud")
    return m


# ---- one call --------------------------------------------------------------------------------------------------------
class _State:
    """device counter + workspaces (one per batch size) of one stream of draws"""

    def __init__(self, seed, device):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        self.counter = None
        self.workspaces = {}

    def buffers(self, b):
        if self.counter is None:
            self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        ws = self.workspaces.get(b)
        if ws is None:
            nbytes = u64_array([0])
            launch("pn2_augment_workspace_bytes", self.device, b, nbytes, stream=False)
            ws = torch.empty(nbytes[0] + 256, dtype=torch.uint8, device=self.device)
            self.workspaces[b] = ws
        return self.counter, ws


def _f64(draws, key, shape, dev):
    a = np.ascontiguousarray(np.asarray(draws[key], dtype=np.float64))
    if a.shape != shape:
        raise ValueError("draws[%r] must have shape %s, not %s" % (key, shape, a.shape))
    return torch.from_numpy(a).to(dev)


def _augment(state, data, flags, axis=None, perturb=None, scale=None, shift=None, jitter=None, dropout=None,
             labels=None, weights=None, out=None, draws=None):
    """one pn2_augment call -> out, out_labels, out_weights, params (B,16) float64, perm (N,) int32 | None"""
    require_cuda(data, labels, weights, out)
    if data.dim() != 3 or data.dtype != torch.float32:
        raise ValueError("the batch must be a (B,N,C) float32 tensor")
    data = data if data.is_contiguous() else data.contiguous()
    b, n, c = data.shape
    dev = data.device
    if out is None:
        out = torch.empty_like(data)
    elif out.shape != data.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 tensor of the batch's shape on its device")
    shuffle = bool(flags & SHUFFLE)
    if shuffle and out.data_ptr() == data.data_ptr():
        raise ValueError("the shuffle cannot work in place")
    lab_out = w_out = None
    if labels is not None:
        if labels.shape != (b, n) or labels.dtype != torch.int32:
            raise ValueError("labels must be (B,N) int32")
        labels = labels.contiguous()
        lab_out = torch.empty_like(labels) if shuffle else labels  # only ever permuted
    if weights is not None:
        if weights.shape != (b, n) or weights.dtype != torch.float32:
            raise ValueError("weights must be (B,N) float32")
        weights = weights.contiguous()
        w_out = torch.empty_like(weights) if shuffle else weights
    d = dict.fromkeys(("perm", "matrix", "scale", "shift", "noise", "ratio", "u"))
    if draws is not None:
        flags |= REPLAY
        if shuffle:
            perm = np.asarray(draws["perm"]).astype(np.int64).reshape(-1)
            if perm.shape != (n,) or not np.array_equal(np.sort(perm), np.arange(n)):
                raise ValueError("draws['perm'] must be a permutation of range(N)")
            d["perm"] = torch.from_numpy(perm.astype(np.int32)).to(dev)
        if flags & (ROTATE | PERTURB):
            d["matrix"] = torch.from_numpy(np.ascontiguousarray(_matrices(b, axis, perturb, draws))).to(dev)
        if flags & SCALE:
            d["scale"] = _f64(draws, "scale", (b,), dev)
        if flags & SHIFT:
            d["shift"] = _f64(draws, "shift", (b, 3), dev)
        if flags & JITTER:
            d["noise"] = _f64(draws, "noise", (b, n, c if flags & JITTER_ALL else 3), dev)
        if flags & DROPOUT:
            d["ratio"], d["u"] = _f64(draws, "ratio", (b,), dev), _f64(draws, "u", (b, n), dev)
    counter, ws = state.buffers(b)
    base = (-ws.data_ptr()) % 256
    params = torch.empty((b, _PARAMS), dtype=torch.float64, device=dev)
    perm_out = torch.empty(n, dtype=torch.int32, device=dev) if shuffle else None
    perturb, scale, jitter = perturb or (0.0, 1.0), scale or (1.0, 1.0), jitter or (0.0, 1.0)
    launch("pn2_augment", dev, b, n, c, flags, _AXES.get(axis, 2), float(perturb[0]), float(perturb[1]), float(scale[0]),
           float(scale[1]), float(shift or 0.0), float(jitter[0]), float(jitter[1]), float(dropout or 0.0), state.seed,
           ptr(counter), ptr(d["perm"]), ptr(d["matrix"]), ptr(d["scale"]), ptr(d["shift"]), ptr(d["noise"]), ptr(d["ratio"]),
           ptr(d["u"]), ptr(data), ptr(labels) if shuffle else None, ptr(weights) if shuffle else None, ptr(ws[base:]),
           ws.numel() - base, ptr(params), ptr(perm_out), ptr(out), ptr(lab_out) if shuffle else None,
           ptr(w_out) if shuffle else None)
    return out, lab_out, w_out, params, perm_out


# ---- the reference's functions -----------------------------------------------------------------------------------------
_SEED = [0]
_DEFAULT = {}


def seed(value):
    """seed of the device draws of the module-level functions (default 0); their batch counters start again at zero"""
    _SEED[0] = int(value)
    _DEFAULT.clear()


def _default(t):
    require_cuda(t)
    st = _DEFAULT.get(t.device)
    if st is None:
        st = _DEFAULT[t.device] = _State(_SEED[0], t.device)
    return st


def _axis(rotation_axis):
    if rotation_axis not in _AXES:
        raise ValueError("Wrong rotation axis")
    return rotation_axis


def shuffle_data(data, labels):
    """Shuffle data and labels along the batch axis -> shuffled data, labels and the indices"""
    idx = torch.randperm(len(labels), device=labels.device)
    return data[idx, ...], labels[idx], idx


def shuffle_points(batch_data, draws=None):
    """Shuffle the order of the points, with the same permutation for the whole batch.  draws: perm"""
    return _augment(_default(batch_data), batch_data, SHUFFLE, draws=draws)[0]


def rotate_point_cloud(batch_data, rotation_axis="z", draws=None):
    """Rotate every (B,N,3) cloud by its own random angle about `rotation_axis`.  draws: angle"""
    if batch_data.dim() != 3:
        raise ValueError("np.ndim(batch_data) != 3, must be (b, n, 3)")
    if batch_data.shape[2] != 3:
        raise ValueError("batch_data.shape[2] != 3, must be (x, y, z)")
    return _augment(_default(batch_data), batch_data, ROTATE, axis=_axis(rotation_axis), draws=draws)[0]


def rotate_feature_point_cloud(batch_data, feature_size=3, rotation_axis="z", draws=None):
    """Rotate the xyz of (B,N,3+feature_size) clouds; the features are copied.  draws: angle"""
    if batch_data.dim() != 3 or batch_data.shape[2] != 3 + feature_size:
        raise ValueError("batch_data must be (b, n, 3 + feature_size)")
    return _augment(_default(batch_data), batch_data, ROTATE, axis=_axis(rotation_axis), draws=draws)[0]


def rotate_point_cloud_with_normal(batch_xyz_normal, draws=None):
    """Rotate xyz and normals (channels 3:6) about y, in place.  draws: angle"""
    return _augment(_default(batch_xyz_normal), batch_xyz_normal, ROTATE | ROTATE_NORMALS, axis="y", out=batch_xyz_normal,
                    draws=draws)[0]


def rotate_perturbation_point_cloud_with_normal(batch_data, angle_sigma=0.06, angle_clip=0.18, draws=None):
    """Perturb xyz and normals by small random rotations.  draws: normals"""
    return _augment(_default(batch_data), batch_data, PERTURB | ROTATE_NORMALS, perturb=(angle_sigma, angle_clip),
                    draws=draws)[0]


def rotate_perturbation_point_cloud(batch_data, angle_sigma=0.06, angle_clip=0.18, draws=None):
    """Perturb (B,N,3) clouds by small random rotations.  draws: normals"""
    return _augment(_default(batch_data), batch_data, PERTURB, perturb=(angle_sigma, angle_clip), draws=draws)[0]


def _by_angle(batch_data, rotation_angle, flags):
    b = batch_data.shape[0]
    return _augment(_default(batch_data), batch_data, flags, axis="y",
                    draws=dict(angle=np.full(b, rotation_angle, dtype=np.float64)))[0]


def rotate_point_cloud_by_angle(batch_data, rotation_angle):
    """Rotate every cloud about y by the given angle"""
    return _by_angle(batch_data, rotation_angle, ROTATE)


def rotate_point_cloud_by_angle_with_normal(batch_data, rotation_angle):
    """Rotate xyz and normals about y by the given angle"""
    return _by_angle(batch_data, rotation_angle, ROTATE | ROTATE_NORMALS)


def jitter_point_cloud(batch_data, sigma=0.01, clip=0.05, draws=None):
    """Add clip(sigma * randn, -clip, clip) to every value (all C channels, as the reference does).  draws: noise (B,N,C)"""
    assert clip > 0
    return _augment(_default(batch_data), batch_data, JITTER | JITTER_ALL, jitter=(sigma, clip), draws=draws)[0]


def shift_point_cloud(batch_data, shift_range=0.1, draws=None):
    """Shift every cloud by its own uniform(-shift_range, shift_range) vector, in place.  draws: shift"""
    return _augment(_default(batch_data), batch_data, SHIFT, shift=shift_range, out=batch_data, draws=draws)[0]


def random_scale_point_cloud(batch_data, scale_low=0.8, scale_high=1.25, draws=None):
    """Scale every cloud by its own uniform(scale_low, scale_high) factor, in place.  draws: scale"""
    return _augment(_default(batch_data), batch_data, SCALE, scale=(scale_low, scale_high), out=batch_data, draws=draws)[0]


def random_point_dropout(batch_pc, max_dropout_ratio=0.875, draws=None):
    """Replace a random share (at most max_dropout_ratio) of every cloud's rows by its first row, in place.  draws: ratio, u"""
    return _augment(_default(batch_pc), batch_pc, DROPOUT, dropout=max_dropout_ratio, out=batch_pc, draws=draws)[0]


# ---- the fused pipeline --------------------------------------------------------------------------------------------------
class Augmenter:
    """Any set of the stages as ONE pn2_augment call, capturable in a graph.  It owns the device batch counter and the
    workspace; under torch.distributed the rank is folded into the seed as the dataset does, so every rank draws its own
    stream.  rotate: "x" | "y" | "z" | None; perturb: (angle_sigma, angle_clip); with both, the cloud's matrix is
    R_axis . R_perturb.  scale: (lo, hi); shift: range; jitter: (sigma, clip), xyz only unless jitter_all_channels;
    dropout: max ratio; shuffle: one permutation per call, labels and weights follow; rotate_normals: channels 3:6 too.
    After a call last_matrix (B,3,3), last_scale (B,), last_shift (B,3), last_ratio (B,) (float64) and last_perm (N,) int32
    (None without shuffle) say what was applied.  One call at a time per object: the workspace is shared between calls."""

    def __init__(self, seed=0, device="cuda", rotate=None, perturb=None, scale=None, shift=None, jitter=None, dropout=None,
                 shuffle=False, rotate_normals=False, jitter_all_channels=False):
        from ..dataset.multi_scene import _rank_seed
        if rotate is not None:
            _axis(rotate)
        self.rotate, self.perturb, self.scale, self.shift = rotate, perturb, scale, shift
        self.jitter, self.dropout, self.shuffle, self.rotate_normals = jitter, dropout, bool(shuffle), bool(rotate_normals)
        self.flags = ((SHUFFLE if shuffle else 0) | (ROTATE if rotate is not None else 0) | (PERTURB if perturb is not None else 0)
                      | (SCALE if scale is not None else 0) | (SHIFT if shift is not None else 0)
                      | (JITTER if jitter is not None else 0) | (DROPOUT if dropout is not None else 0)
                      | (ROTATE_NORMALS if rotate_normals else 0) | (JITTER_ALL if jitter_all_channels else 0))
        self.seed = _rank_seed(seed)
        self.device = torch.device(device)
        self._state = _State(self.seed, self.device)
        self.last_matrix = self.last_scale = self.last_shift = self.last_ratio = self.last_perm = None

    @property
    def batch_counter(self):
        """device int64 (1,): calls drawn so far from the device random numbers"""
        return self._state.buffers(1)[0]

    def __call__(self, data, labels=None, weights=None, out=None, draws=None):
        """-> the augmented batch; with labels and / or weights: (batch, labels, weights) (None where none was given)"""
        out, lab, w, params, perm = _augment(self._state, data, self.flags, axis=self.rotate, perturb=self.perturb,
                                             scale=self.scale, shift=self.shift, jitter=self.jitter, dropout=self.dropout,
                                             labels=labels, weights=weights, out=out, draws=draws)
        self.last_matrix, self.last_scale = params[:, :9].reshape(-1, 3, 3), params[:, 9]
        self.last_shift, self.last_ratio, self.last_perm = params[:, 10:13], params[:, 13], perm
        if labels is None and weights is None:
            return out
        return out, lab, w
