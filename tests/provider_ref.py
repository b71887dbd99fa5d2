"""numpy model of pn2_augment (include/pn2_abi.h, "point-cloud augmentation"), used by the tests only.  Written from the rule the
header documents, not from the kernel: stage order, float64 between enabled stages with ONE rounding to float32, the plain
order of the rotation's three products, dropout's row-0 rule, and -- for the device mode -- the tags, the uniform, the
Box-Muller normal and the key-rank permutation of its counter-based stream (hashes: tests/dataset_stream_ref.py).

A configuration is a dict with any of: shuffle (bool), rotate ("x" | "y" | "z"), perturb (sigma, clip), normals (bool),
scale (lo, hi), shift (range), jitter (sigma, clip), jitter_all (bool), dropout (max ratio).  In replay only the presence of a
key matters for rotate / perturb / scale / shift / dropout; jitter's sigma and clip are always read.
Draws: perm (N,), matrix (B,3,3), scale (B,), shift (B,3), noise (B,N,cj), ratio (B,), u (B,N)."""
import numpy as np

import dataset_stream_ref as S

_U = np.uint64
T = 2 ** 41
TAG_ANGLE, TAG_PERTURB, TAG_SCALE, TAG_SHIFT, TAG_RATIO = T, T + 2, T + 8, T + 9, T + 12
TAG_JITTER, TAG_DROP, TAG_PERM = 2 * T, 4 * T, 8 * T


# ---- arithmetic --------------------------------------------------------------------------------------------------------
def rotate_rows(p, r):
    """p (..., 3) float64 @ r (3,3): (x * r[0][j] + y * r[1][j]) + z * r[2][j], every operation rounded on its own"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([(x * r[0, j] + y * r[1, j]) + z * r[2, j] for j in range(3)], -1)


def mat3(a, b):
    """a . b (3,3) in the plain order (a0 * b0 + a1 * b1) + a2 * b2"""
    return np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)])


def apply(x, cfg, draws, labels=None, weights=None):
    """the pipeline on a float32 batch x (B,N,C) -> float32 (B,N,C) [, labels, weights]"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    b, n, c = x.shape
    rot = "rotate" in cfg or "perturb" in cfg
    v = x.astype(np.float64)
    if cfg.get("shuffle"):
        perm = np.asarray(draws["perm"])
        v = v[:, perm, :]
        labels = None if labels is None else labels[:, perm]
        weights = None if weights is None else weights[:, perm]
    for s in range(b):
        if rot:
            r = np.asarray(draws["matrix"][s], dtype=np.float64)
            v[s, :, 0:3] = rotate_rows(v[s, :, 0:3], r)
            if cfg.get("normals"):
                v[s, :, 3:6] = rotate_rows(v[s, :, 3:6], r)
        if "scale" in cfg:
            v[s, :, 0:3] = v[s, :, 0:3] * np.float64(draws["scale"][s])
        if "shift" in cfg:
            v[s, :, 0:3] = v[s, :, 0:3] + np.asarray(draws["shift"][s], dtype=np.float64)
    if "jitter" in cfg:
        sigma, clip = cfg["jitter"]
        cj = c if cfg.get("jitter_all") else 3
        noise = np.asarray(draws["noise"], dtype=np.float64)
        assert noise.shape == (b, n, cj)
        v[:, :, :cj] = v[:, :, :cj] + np.clip(sigma * noise, -1 * clip, clip)
    out = v.astype(np.float32)  # the one rounding
    if "dropout" in cfg:
        for s in range(b):
            dropped = np.asarray(draws["u"][s]) <= draws["ratio"][s]
            out[s, dropped, :] = out[s, 0, :]  # row 0 as it leaves stage 4; row 0 itself keeps its value
    if labels is None and weights is None:
        return out
    return out, labels, weights


# ---- the device stream -------------------------------------------------------------------------------------------------
def unit(h, i):
    """draw i (an int or an array of ints) of stream h as a float64 in [0, 1)"""
    return S.unit53(S.draw64(h, np.asarray(i, dtype=np.uint64).reshape(-1)))


def uniform(lo, hi, u):
    return lo + (hi - lo) * u


def normal(h, i):
    """Box-Muller in float64 from the draws i and i + 1"""
    i = np.asarray(i, dtype=np.uint64).reshape(-1)
    u1, u2 = unit(h, i), unit(h, i + _U(1))
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos((u2 * 2.0) * np.pi)


def axis_matrix(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    return {"x": np.array([[1, 0, 0], [0, c, s], [0, -s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])}[axis]


def perturb_matrix(angles):
    a = angles
    rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    return mat3(rz, mat3(ry, rx))


def permutation(seed, counter, n):
    """the indices sorted by (key, index); keys from the stream of cloud index -1"""
    h = S.sample_stream(seed, counter, -1)
    keys = S.draw64(h, np.arange(n, dtype=np.uint64) + _U(TAG_PERM))
    return np.lexsort((np.arange(n), keys)).astype(np.int32)


def device_draws(cfg, seed, counter, b, n, c):
    """every draw of the call made at batch counter `counter`, in the replay mode's form"""
    d = {}
    if cfg.get("shuffle"):
        d["perm"] = permutation(seed, counter, n)
    cj = c if cfg.get("jitter_all") else 3
    d["matrix"] = np.tile(np.eye(3), (b, 1, 1))
    d["scale"], d["shift"], d["ratio"] = np.ones(b), np.zeros((b, 3)), np.zeros(b)
    for s in range(b):
        h = S.sample_stream(seed, counter, s)
        r = None
        if "rotate" in cfg:
            r = axis_matrix(cfg["rotate"], float((unit(h, TAG_ANGLE)[0] * 2.0) * np.pi))
        if "perturb" in cfg:
            sigma, clip = cfg["perturb"]
            rp = perturb_matrix(np.clip(sigma * normal(h, [TAG_PERTURB, TAG_PERTURB + 2, TAG_PERTURB + 4]), -clip, clip))
            r = rp if r is None else mat3(r, rp)
        if r is not None:
            d["matrix"][s] = r
        if "scale" in cfg:
            d["scale"][s] = uniform(cfg["scale"][0], cfg["scale"][1], unit(h, TAG_SCALE)[0])
        if "shift" in cfg:
            rng = float(cfg["shift"])
            d["shift"][s] = uniform(-rng, rng, unit(h, [TAG_SHIFT, TAG_SHIFT + 1, TAG_SHIFT + 2]))
        if "jitter" in cfg:
            at = np.arange(n * cj, dtype=np.uint64)
            d.setdefault("noise", np.empty((b, n, cj)))[s] = normal(h, _U(TAG_JITTER) + _U(2) * at).reshape(n, cj)
        if "dropout" in cfg:
            d["ratio"][s] = unit(h, TAG_RATIO)[0] * cfg["dropout"]
            d.setdefault("u", np.empty((b, n)))[s] = unit(h, np.arange(n, dtype=np.uint64) + _U(TAG_DROP))
    return d


def device_call(x, cfg, seed, counter, labels=None, weights=None):
    """-> (apply(...) of the call made at `counter`, its draws)"""
    b, n, c = x.shape
    d = device_draws(cfg, seed, counter, b, n, c)
    return apply(x, cfg, d, labels, weights), d
