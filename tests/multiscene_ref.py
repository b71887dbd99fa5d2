"""numpy restatement of the reference's multi-scene batch (SemanticDataset.sample_batch_in_all_files / sample_in_all_files,
SemanticFileData.sample and util/provider.py rotate_feature_point_cloud / rotate_point_cloud), used by the tests only.

Every np.random draw goes through `Recorder`, so a batch can be replayed on the device from the recorded draws, and
`synthetic_scenes` regenerates the fixture's scenes from seeds (tests/golden/multiscene_sampler.npz stores no scene)."""
import numpy as np

# (seed, points, x extent, y extent): dense and sparse scenes, so that with box 4 and N = 256 columns hold more and fewer
# than N points
FIXTURE_SCENES = [(11, 20000, 30.0, 20.0), (12, 3000, 25.0, 25.0), (13, 8000, 20.0, 20.0), (14, 12000, 40.0, 10.0)]


def synthetic_scene(seed, n, ex, ey):
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.uniform(0, ex, n), rs.uniform(0, ey, n), np.abs(rs.normal(0, 2.0, n))], 1)
    pts = pts.astype(np.float32).astype(np.float64)  # what a float32 .pcd gives Open3D
    labels = rs.randint(0, 9, n).astype(np.int32)
    colors = rs.randint(0, 256, (n, 3)) / 255.0
    return pts, labels, colors


def synthetic_scenes(spec=FIXTURE_SCENES):
    return [synthetic_scene(*s) + ("scene%d" % i,) for i, s in enumerate(spec)]


class Recorder:
    """np.random stand-in: draws from the global numpy stream and keeps what it drew."""

    def __init__(self):
        self.scene, self.center, self.masks, self.angle = [], [], [], []

    def choice(self, a, p=None):
        v = np.random.choice(a, p=p)
        self.scene.append(int(v))
        return v

    def randint(self, lo, hi):
        v = np.random.randint(lo, hi)
        self.center.append(int(v))
        return v

    def shuffle(self, x):
        np.random.shuffle(x)
        self.masks.append((len(self.center) - 1, np.array(x, dtype=np.uint8)))

    def uniform(self):
        v = np.random.uniform()
        self.angle.append(v * 2 * np.pi)
        return v

    def draws(self, batch_size):
        cap = max([len(m) for _, m in self.masks] + [1])
        masks = np.zeros((batch_size, cap), dtype=np.uint8)
        for s, m in self.masks:
            masks[s, :len(m)] = m
        angle = np.array(self.angle if self.angle else [0.0] * batch_size, dtype=np.float64)
        return dict(scene=np.array(self.scene), center=np.array(self.center), masks=masks, angle=angle)


class HostDataset:
    """the x-sorted scenes, probabilities and label weights of a SemanticDataset (host attributes only)"""

    def __init__(self, ds):
        self.points, self.labels, self.colors = ds.scene_points, ds.scene_labels, ds.scene_colors
        self.probas = ds.scene_probas
        self.label_weights = ds.label_weights
        self.hx, self.hy = ds.box_size_x / 2, ds.box_size_y / 2
        self.use_color = ds.use_color
        self.n = ds.num_points_per_sample


def column(points, center_point, hx, hy):
    """_extract_z_box (semantic_dataset.py:123-163): boolean mask of the column around center_point"""
    zs = np.max(points, axis=0)[2] - np.min(points, axis=0)[2]
    lo = center_point - [hx, hy, zs]
    hi = center_point + [hx, hy, zs]
    i0, i1 = np.searchsorted(points[:, 0], lo[0]), np.searchsorted(points[:, 0], hi[0])
    m = np.sum((points[i0:i1] >= lo) * (points[i0:i1] <= hi), axis=1) == 3
    return np.hstack((np.zeros(i0, dtype=bool), m, np.zeros(len(points) - i1, dtype=bool)))


def fixed_size_mask(cnt, n, rnd):
    if cnt - n > 0:
        m = np.concatenate((np.ones(n, dtype=bool), np.zeros(cnt - n, dtype=bool)))
        rnd.shuffle(m)
        return m
    m = np.arange(cnt)
    while len(m) < n:
        m = np.concatenate((m, m))
    return m[:n]


def center_box(p, hx, hy):
    bmin = np.min(p, axis=0)
    return p - np.array([bmin[0] + hx, bmin[1] + hy, bmin[2]])


def rotation(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])


def sample_batch(h, batch_size, augment, rnd):
    """-> batch_data, batch_label, batch_weights exactly as the reference returns them (float64 data without augment)"""
    data, lab, wts = [], [], []
    for _ in range(batch_size):
        k = rnd.choice(np.arange(0, len(h.points)), p=list(h.probas))
        pts, labels, colors = h.points[k], h.labels[k], h.colors[k]
        m = column(pts, pts[rnd.randint(0, len(pts))], h.hx, h.hy)
        p, l, c = pts[m], labels[m], colors[m]
        sm = fixed_size_mask(len(p), h.n, rnd)
        p, l, c = p[sm], l[sm], c[sm]
        pc = center_box(p, h.hx, h.hy)
        data.append(np.hstack((pc, c)) if h.use_color else pc)
        lab.append(l)
        wts.append(h.label_weights[l])
    data, lab, wts = np.array(data), np.array(lab), np.array(wts)
    if augment:
        out = np.zeros(data.shape, dtype=np.float32)
        if h.use_color:
            out[:, :, 3:6] = data[:, :, 3:6]
        for k in range(batch_size):
            ang = rnd.uniform() * 2 * np.pi
            out[k, :, 0:3] = np.dot(data[k, :, 0:3].reshape((-1, 3)), rotation(ang))
        data = out
    return data, lab, wts
