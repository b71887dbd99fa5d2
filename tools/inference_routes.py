"""Which entry points the inference SA / FP modules reach, and what they compute, at the smallest shapes on both sides of every
routing threshold of util/pointnet_util.py (sa_features_inference, dense_mlp_inference).

    python tools/inference_routes.py > profiles/rNN_inference_routes_<what>.txt

Per case: the traced (entry point, numeric arguments) sequence of one module call and the sha256 of its output tensor.  Only the
public layer API (pointnet_sa_module, pointnet_sa_module_msg, pointnet_fp_module with nn given) and _lib.lib.trace are used, so
the same file runs on an older checkout: two outputs that are equal line for line mean the same launches with the same
arguments and the same bits, i.e. the same routes and the same weight preparation (fold, rotate, pad, split).
tests/test_inference_routes_gpu.py pins the entry-point sequences of the same cases (no hashes: a later change of summation
order stays possible).
"""
import contextlib
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, N, K = 2, 1024, 32  # unless a case says otherwise: clouds, source points per cloud, neighbours


def _sa(name, mlp, c, m, k=K, dtype="float32", cols=False, **switches):
    return dict(kind="sa", name=name, mlp=mlp, c=c, m=m, k=k, dtype=dtype, cols=cols, switches=switches)


def _fp(name, mlp, c2, c1, n, cols=False, **switches):
    return dict(kind="fp", name=name, mlp=mlp, c2=c2, c1=c1, n=n, cols=cols, switches=switches)


def _cases():
    out = [
        _sa("sa_32_32_64_c3_dense", [32, 32, 64], 3, 256),
        _sa("sa_32_32_64_c3_column_blocks", [32, 32, 64], 3, 256, cols=True),
        _sa("sa_64_64_128_c64_hoisted", [64, 64, 128], 64, 256),
        _sa("sa_64_64_128_c64_unhoisted", [64, 64, 128], 64, 256, USE_HOISTED_SA=False),
        _sa("sa_128_128_256_c128", [128, 128, 256], 128, 64),
    ]
    for m in (64, 32):  # b * m * 32 = 4096 = WIDE_MIN_ROWS, and 2048 below it
        out.append(_sa("sa_256_256_512_c256_rows%d_hoisted" % (B * m * 32), [256, 256, 512], 256, m))
        out.append(_sa("sa_256_256_512_c256_rows%d_unhoisted" % (B * m * 32), [256, 256, 512], 256, m, USE_HOISTED_SA=False))
    out += [
        _sa("sa_64_64_128_c64_k64", [64, 64, 128], 64, 256, k=64),
        _sa("sa_64_64_128_c64_k48", [64, 64, 128], 64, 256, k=48),
        _sa("sa_64_64_128_bf16_c64", [64, 64, 128], 64, 256, dtype="bfloat16"),
        _sa("sa_64_64_128_bf16_c8", [64, 64, 128], 8, 256, dtype="bfloat16"),
        _sa("sa_32_32_64_c3_fused_off", [32, 32, 64], 3, 256, USE_FUSED_SA=False),
        dict(kind="msg", name="msg_two_scales_c64", mlps=[[32, 32, 64], [64, 64, 128]], ks=[16, 32], c=64, m=256, switches={}),
    ]
    for rows in (65536, 65536 + 32, 65536 - 32):
        out.append(_fp("fp_128x3_c2_128_c1_3_rows%d_hoisted" % rows, [128, 128, 128], 128, 3, rows // B))
        out.append(_fp("fp_128x3_c2_128_c1_3_rows%d_unhoisted" % rows, [128, 128, 128], 128, 3, rows // B, USE_HOISTED_FP=False))
    out.append(_fp("fp_128x3_c2_128_c1_3_rows65536_column_block", [128, 128, 128], 128, 3, 65536 // B, cols=True))
    for rows in (4096, 4032):
        out.append(_fp("fp_256x2_c2_256_c1_128_rows%d" % rows, [256, 256], 256, 128, rows // B))
        out.append(_fp("fp_256x2_c2_256_no_points1_rows%d" % rows, [256, 256], 256, 0, rows // B))
    out += [
        _fp("fp_128x3_rows65536_chain_off", [128, 128, 128], 128, 3, 65536 // B, USE_MLP_CHAIN=False),
        _fp("fp_256x2_c1_128_rows4096_wide_off", [256, 256], 256, 128, 4096 // B, USE_MLP_WIDE=False),
        _fp("fp_128x3_rows65536_fused_fp_off", [128, 128, 128], 128, 3, 65536 // B, USE_FUSED_FP=False),
        _fp("fp_256x2_c1_128_rows4096_fused_fp_off", [256, 256], 256, 128, 4096 // B, USE_FUSED_FP=False),
    ]
    return out


CASES = _cases()


@contextlib.contextmanager
def _switched(pu, switches):
    """module-level A/B switches of pointnet_util set for one case, restored whatever happens"""
    old = {k: getattr(pu, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(pu, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(pu, k, v)


def _randomize_bn(store, seed):
    """non-trivial batch-norm statistics and biases: the fold changes every weight"""
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


def _module_call(pn2, case, dev, seed):
    """-> a function of no arguments that runs the case's module once and returns its feature tensor"""
    pu = pn2.util.pointnet_util
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    if case["kind"] in ("sa", "msg"):
        c = case["c"]
        cloud = t(rs.random_sample((B, N, 3 + c)).astype(np.float32))
        if case.get("cols"):  # the two column blocks of one (b, n, 3 + c) batch, read where they lie
            xyz, pts = cloud[:, :, 0:3], cloud[:, :, 3:]
        else:
            xyz, pts = cloud[:, :, 0:3].contiguous(), cloud[:, :, 3:].contiguous()
        if case.get("dtype") == "bfloat16":
            pts = pts.to(torch.bfloat16)
        if case["kind"] == "msg":
            return lambda: pu.pointnet_sa_module_msg(xyz, pts, case["m"], [0.1, 0.2], case["ks"], case["mlps"], False, None,
                                                     "mod")[1]
        return lambda: pu.pointnet_sa_module(xyz, pts, npoint=case["m"], radius=0.2, nsample=case["k"], mlp=case["mlp"], mlp2=None,
                                             group_all=False, is_training=False, bn_decay=None, scope="mod")[1]
    n, c1, c2 = case["n"], case["c1"], case["c2"]
    xyz1 = t(rs.random_sample((B, n, 3)).astype(np.float32))
    xyz2 = t(rs.random_sample((B, N, 3)).astype(np.float32))
    dist = t((rs.random_sample((B, n, 3)) * 0.01 + 1e-4).astype(np.float32))
    idx = t(rs.randint(0, N, (B, n, 3)).astype(np.int32))
    p2 = t(rs.randn(B, N, c2).astype(np.float32))
    p1 = None
    if c1:
        if case["cols"]:
            p1 = t(rs.randn(B, n, 3 + c1).astype(np.float32))[:, :, 3:]
        else:
            p1 = t(rs.randn(B, n, c1).astype(np.float32))
    return lambda: pu.pointnet_fp_module(xyz1, xyz2, p1, p2, case["mlp"], False, None, "mod", nn=(dist, idx))


def run_case(pn2, case, dev, seed=0):
    """-> ([(entry point, numeric args)], sha256 of the output) of one traced module call"""
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    store = tfu.set_default_store(tfu.VariableStore(device=dev, seed=seed))
    call = _module_call(pn2, case, dev, seed + 1)
    with _switched(pu, case["switches"]), torch.no_grad():
        call()  # creates the variables
        _randomize_bn(store, seed + 2)
        pn2._lib.lib.trace = calls = []
        try:
            out = call()
        finally:
            pn2._lib.lib.trace = None
    torch.cuda.synchronize()
    raw = out.detach().contiguous().cpu().view(torch.uint8 if out.dtype != torch.float32 else torch.float32).numpy().tobytes()
    return [(c[0], tuple(c[1])) for c in calls], hashlib.sha256(raw).hexdigest()


def main():
    import pn2_amd as pn2
    dev = torch.device("cuda:0")
    for i, case in enumerate(CASES):
        calls, digest = run_case(pn2, case, dev, seed=100 + i)
        print("case %s" % case["name"])
        for name, args in calls:
            print("  %s %s" % (name, " ".join(repr(a) for a in args)))
        print("  sha256 %s" % digest)


if __name__ == "__main__":
    main()
