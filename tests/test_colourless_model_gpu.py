"""The SA x4 + FP x4 stack and the head with use_color = 0 (the reference's semantic_no_color.json, the configuration its KITTI
predictor loads) against the float64 oracle: the coloured stack test of tests/test_layers_gpu.py with l0_points = None, so SA1
groups xyz only and FP4 has no skip link.  Tolerance: |hip - ref64| <= 1e-5 + 1e-5 |ref64| on the features (the project's
north-star bound, the one the coloured stack test uses), 5e-5 + 5e-5 |ref64| on the logits (as the coloured head test)."""
import numpy as np
import pytest

from conftest import s_scene

pytestmark = pytest.mark.gpu


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def randomize_bn(store, seed):
    """non-trivial BN statistics so that folding is actually exercised"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in store.params.items():
            if k.endswith("bn/gamma"):
                v.copy_((torch.rand(v.shape, generator=g) + 0.5).to(v.device))
            elif k.endswith("bn/beta") or k.endswith("biases"):
                v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
        for k, v in store.buffers.items():
            if k.endswith("moving_mean"):
                v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
            elif k.endswith("moving_variance"):
                v.copy_((torch.rand(v.shape, generator=g) + 0.5).to(v.device))


def layer_dicts(store, scope, names, bn=True):
    out = []
    for nm in names:
        p = ("%s/" % scope if scope else "") + nm + "/"
        W = store.params[p + "weights"].detach().cpu().numpy().astype(np.float64)
        W = W.reshape(W.shape[-2], W.shape[-1])
        d = dict(W=W, b=store.params[p + "biases"].detach().cpu().numpy())
        if bn:
            d.update(gamma=store.params[p + "bn/gamma"].detach().cpu().numpy(),
                     beta=store.params[p + "bn/beta"].detach().cpu().numpy(),
                     mean=store.buffers[p + "bn/moving_mean"].cpu().numpy(),
                     var=store.buffers[p + "bn/moving_variance"].cpu().numpy())
        out.append(d)
    return out


def oracle_stack(oracle, store, xyz, hp, pn2):
    """model.py:30-129 with l0_points = None, in float64"""
    xyzs, feats = [xyz], [None]
    for li in range(4):
        k = "l%d_" % (li + 1)
        layers = layer_dicts(store, "layer%d" % (li + 1), ["conv%d" % i for i in range(3)])
        points = None if feats[-1] is None else feats[-1].astype(np.float32)
        nx, npts, _ = oracle.sa_module(xyzs[-1], points, hp[k + "npoint"], hp[k + "radius"], hp[k + "nsample"], layers)
        xyzs.append(nx)
        feats.append(npts)
    up = feats[4]
    for fi in range(4):
        lvl = 3 - fi
        names = ["conv_%d" % i for i in range(len(pn2.model.FP_MLPS[fi]))]
        layers = layer_dicts(store, "fa_layer%d" % (fi + 1), names)
        skip = None if feats[lvl] is None else feats[lvl].astype(np.float32)
        up = oracle.fp_module(xyzs[lvl], xyzs[lvl + 1], skip, up.astype(np.float32), layers)
    return up


def test_colourless_stack_and_head_vs_oracle(pn2, oracle, cuda):
    tfu = pn2.util.tf_util
    hp = dict(pn2.model.SEMANTIC_NO_COLOR_HYPERPARAMS)
    hp.update(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)
    assert hp["use_color"] == 0
    xyz = np.asarray(s_scene(1, 2, 2048))
    store = tfu.set_default_store(tfu.VariableStore(device=cuda, seed=11))
    pn2.model.get_model(T(xyz, cuda), False, 9, hp)  # creates the variables
    assert tuple(store.params["layer1/conv0/weights"].shape)[-2] == 3  # SA1 sees xyz only
    randomize_bn(store, 12)
    out, _ = pn2.model.get_sa_fp_features(T(xyz, cuda), False, hp)
    logits, _ = pn2.model.get_model(T(xyz, cuda), False, 9, hp)
    ref = oracle_stack(oracle, store, xyz, hp, pn2)
    assert out.shape == (2, 2048, 128)
    got = out.cpu().numpy()
    err = np.abs(got - ref)
    print("colourless small stack end-to-end err %.2e of (1+|ref|)" % (err / (1 + np.abs(ref))).max())
    assert (err <= 1e-5 + 1e-5 * np.abs(ref)).all(), err.max()
    (fc1,) = layer_dicts(store, None, ["fc1"])
    (fc2,) = layer_dicts(store, None, ["fc2"], bn=False)
    ref_logits = oracle.model_head(ref, fc1, fc2)
    herr = np.abs(logits.cpu().numpy().astype(np.float64) - ref_logits)
    print("colourless logits err %.2e" % herr.max())
    assert logits.shape == (2, 2048, 9) and (herr <= 5e-5 + 5e-5 * np.abs(ref_logits)).all(), herr.max()
