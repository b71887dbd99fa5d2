"""Shared inputs of tests/test_provider_cpu.py and tests/test_provider_gpu.py: the golden cases of tests/golden/provider.npz
(the reference's util/provider.py, frozen by tests/golden/make_provider_golden.py) and the seeded edge-shape draws."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "provider.npz")

# shapes of the edge tests: the lane, wave and workgroup edges and the odd row widths
BATCHES, POINTS, CHANNELS = (1, 3), (1, 63, 64, 65, 257, 1000), (3, 6, 7)


def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def _axis_matrices(axis, angles):
    out = []
    for a in angles:
        c, s = np.cos(a), np.sin(a)
        out.append({"x": [[1, 0, 0], [0, c, s], [0, -s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                    "z": [[c, s, 0], [-s, c, 0], [0, 0, 1]]}[axis])
    return np.array(out, dtype=np.float64)


def _perturb_matrices(normals, sigma, clip):
    out = []
    for g in normals:
        a = np.clip(sigma * g, -clip, clip)
        rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        out.append(np.dot(rz, np.dot(ry, rx)))  # the matrix itself is the reference's np.dot: it is an INPUT of the replay
    return np.array(out)


def golden_cases(g):
    """-> [(case, input key, model configuration, model draws, package function name, its arguments, its draws)]"""
    b = g["in3"].shape[0]
    cases = [("shuffle", "in6", {"shuffle": True}, {"perm": g["shuffle_perm"]}, "shuffle_points", (), {"perm": g["shuffle_perm"]})]
    for axis in "xyz":
        a = g["rotate_%s_angle" % axis]
        cases.append(("rotate_" + axis, "in3", {"rotate": axis}, {"matrix": _axis_matrices(axis, a)}, "rotate_point_cloud",
                      (axis,), {"angle": a}))
    a = g["rotate_feature_angle"]
    cases.append(("rotate_feature", "in6", {"rotate": "z"}, {"matrix": _axis_matrices("z", a)}, "rotate_feature_point_cloud",
                  (3, "z"), {"angle": a}))
    a = g["rotate_normal_angle"]
    cases.append(("rotate_normal", "in6", {"rotate": "y", "normals": True}, {"matrix": _axis_matrices("y", a)},
                  "rotate_point_cloud_with_normal", (), {"angle": a}))
    z = g["perturb_normals"]
    cases.append(("perturb", "in3", {"perturb": (0.06, 0.18)}, {"matrix": _perturb_matrices(z, 0.06, 0.18)},
                  "rotate_perturbation_point_cloud", (), {"normals": z}))
    z = g["perturb_normal_normals"]
    cases.append(("perturb_normal", "in6", {"perturb": (0.06, 0.18), "normals": True},
                  {"matrix": _perturb_matrices(z, 0.06, 0.18)}, "rotate_perturbation_point_cloud_with_normal", (), {"normals": z}))
    ang = float(g["by_angle_angle"][0])
    cases.append(("by_angle", "in3", {"rotate": "y"}, {"matrix": _axis_matrices("y", np.full(b, ang))},
                  "rotate_point_cloud_by_angle", (ang,), None))
    cases.append(("jitter", "in3", {"jitter": (0.01, 0.05), "jitter_all": True}, {"noise": g["jitter_noise"]},
                  "jitter_point_cloud", (), {"noise": g["jitter_noise"]}))
    cases.append(("shift", "in3", {"shift": 0.1}, {"shift": g["shift_shift"]}, "shift_point_cloud", (), {"shift": g["shift_shift"]}))
    cases.append(("scale", "in3", {"scale": (0.8, 1.25)}, {"scale": g["scale_scale"]}, "random_scale_point_cloud", (),
                  {"scale": g["scale_scale"]}))
    for case, key, mx in (("dropout", "in6", 0.875), ("dropout_none", "in3", 0.004)):
        d = {"ratio": g[case + "_ratio"], "u": g[case + "_u"]}
        cases.append((case, key, {"dropout": mx}, d, "random_point_dropout", (mx,), d))
    return cases


# ---- edge shapes: seeded draws in the replay mode's form ---------------------------------------------------------------------
STAGES = {  # one stage at a time, then everything fused
    "shuffle": {"shuffle": True},
    "rotate": {"rotate": "z"},
    "rotate_normals": {"rotate": "y", "perturb": (0.06, 0.18), "normals": True},
    "scale": {"scale": (0.8, 1.25)},
    "shift": {"shift": 0.1},
    "jitter": {"jitter": (0.01, 0.05)},
    "jitter_all": {"jitter": (0.01, 0.05), "jitter_all": True},
    "dropout": {"dropout": 0.875},
    "fused": {"shuffle": True, "rotate": "z", "perturb": (0.06, 0.18), "scale": (0.8, 1.25), "shift": 0.1,
              "jitter": (0.01, 0.05), "dropout": 0.875},
}


def edge_input(b, n, c, seed=0):
    rs = np.random.RandomState(1000 * seed + 97 * b + 7 * n + c)
    x = rs.uniform(-5, 5, (b, n, c)).astype(np.float32)
    labels = rs.randint(0, 9, (b, n)).astype(np.int32)
    weights = rs.uniform(0, 2, (b, n)).astype(np.float32)
    return x, labels, weights


def edge_draws(b, n, c, cfg, seed=0):
    """draws of every stage of cfg.  Dropout: cloud 0 drops row 0 and about half of its rows; with b == 3, cloud 1 has ratio 0
    (and u[1][5] == 0.0: `<=` drops exactly that row) and cloud 2 a ratio above every u (every row becomes row 0)."""
    rs = np.random.RandomState(5000 * seed + 13 * b + 3 * n + c)
    d = {"perm": rs.permutation(n).astype(np.int32)}
    ang = rs.uniform(0, 2 * np.pi, b)
    d["matrix"] = _axis_matrices(cfg.get("rotate", "z"), ang)
    if "perturb" in cfg:
        rp = _perturb_matrices(rs.randn(b, 3), *cfg["perturb"])
        d["matrix"] = np.array([np.dot(d["matrix"][k], rp[k]) for k in range(b)]) if "rotate" in cfg else rp
    d["scale"] = rs.uniform(0.8, 1.25, b)
    d["shift"] = rs.uniform(-0.1, 0.1, (b, 3))
    d["noise"] = rs.randn(b, n, c if cfg.get("jitter_all") else 3)
    d["ratio"] = np.full(b, 0.5)
    d["u"] = rs.random_sample((b, n))
    d["u"][0, 0] = 0.25
    if b == 3:
        d["ratio"][1], d["ratio"][2] = 0.0, 1.5
        if n > 5:
            d["u"][1, 5] = 0.0
    return d
