"""Which entry points one training forward + backward of the SA / MSG / FP modules and the dense layers reaches, with what numeric
arguments, and what it computes -- at the smallest shapes on both sides of every host-side threshold of the training layer path
(util/tf_util.py: can_defer_bn, HOIST_BN_STATS_MIN_ROWS, the narrow fused backward, the on-load batch-norm gradient, the column
block split; util/pointnet_util.py: the first-layer forms) and with every training switch off, one at a time.

    python tools/training_routes.py [--full] [--save run.npz] [--against first_run.npz] > profiles/rNN_training_routes_<what>.txt
    python tools/training_routes.py --check parent.txt parent_again.txt head.txt

Per case two lines.  `launches`: how many, a sha256 (16 hex digits) over the traced "entry point, numeric arguments" lines, forward
then backward in the autograd engine's order, and the entry points (--full prints the lines themselves below: where two digests
differ, diff those).  `tensors`: label:sha256 (12 hex digits) of the output, of the gradient of every input that requires one, of
every parameter gradient and of the moving averages (as one tensor); --against appends, where the bytes differ from the same
tensor of an earlier run (--save), :the largest absolute difference relative to that tensor's largest magnitude -- weight
gradients are accumulated with atomics, so not every hash repeats.  Only the public layer API and _lib.lib.trace are used, so the
same file runs on an older checkout.  --check compares three outputs (an older checkout twice, this one once): launches lines
equal; hashes the older checkout repeats equal; the others within twice the older checkout's own figure.
tests/test_training_routes_gpu.py pins the entry-point sequences of the same cases.
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

B, N, K = 2, 1024, 32  # clouds, source points per cloud, neighbours (unless a case says otherwise)

SWITCHES = ("USE_GEMM_BN_STATS", "USE_BN_FINISH_IN_PRODUCER", "USE_DGRAD_BN_STATS", "USE_BN_ON_LOAD", "USE_BN_GRAD_ON_LOAD",
            "USE_POOLED_BN_REDUCE", "USE_FUSED_BWD_NARROW", "USE_SA_FIRST_LAYER_FUSED", "USE_HOIST_BN_STATS", "USE_HOISTED_TRAIN",
            "USE_HOISTED_MSG_TRAIN")


def _sa(name, mlp, c, m, geo="none", pooling="max", no_grad=False):
    """geo: "none" (FPS + ball query inside the module), "idx" (given ahead), "plan" (+ the scatter plan)"""
    return dict(kind="sa", name=name, mlp=mlp, c=c, m=m, geo=geo, pooling=pooling, no_grad=no_grad, switches={})


def _msg(name, mlps, geo=True):
    return dict(kind="msg", name=name, mlps=mlps, ks=[16, 32], c=64, m=64, geo=geo, switches={})


def _fp(name, c1, plan, defer_last=0):
    return dict(kind="fp", name=name, mlp=[128, 128, 128], c2=128, c1=c1, n=2048, plan=plan, defer_last=defer_last, switches={})


def _stack(name, rows, cin, widths, **kw):
    """kw: bn (True), conv1d (False), fanout (False: a chain; True: the first layer's output feeds the other two)"""
    return dict(kind="stack", name=name, rows=rows, cin=cin, widths=widths, switches={}, **kw)


def _base_cases():
    return [
        # b * m * 32 rows: 4096 is above can_defer_bn's 2048, 2048 is not
        _sa("sa_c3_32_32_64_rows4096", [32, 32, 64], 3, 64),
        _sa("sa_c3_32_32_64_rows2048", [32, 32, 64], 3, 32),
        _sa("sa_c3_64_pooled_first", [64], 3, 64),
        _sa("sa_c64_64_64_128_plan_rows4096", [64, 64, 128], 64, 64, geo="plan"),
        _sa("sa_c64_64_64_128_plan_rows32768", [64, 64, 128], 64, 512, geo="plan"),  # = HOIST_BN_STATS_MIN_ROWS
        _sa("sa_c64_64_64_128_plan_rows32704", [64, 64, 128], 64, 511, geo="plan"),
        _sa("sa_c64_64_64_128_idx_only", [64, 64, 128], 64, 64, geo="idx"),
        _sa("sa_c8_32_32_64_grouped", [32, 32, 64], 8, 64),
        _sa("sa_c8_32_32_64_avg", [32, 32, 64], 8, 64, pooling="avg"),
        _msg("msg_two_scales_hoisted", [[32, 32, 64], [64, 64, 128]]),
        _msg("msg_one_layer_scale_hoisted", [[64], [64, 128]]),
        _msg("msg_two_scales_no_geometry", [[32, 32, 64], [64, 64, 128]], geo=False),
        _fp("fp_c1_3_plan_defer_last_128", 3, True, 128),
        _fp("fp_c1_3_plan", 3, True),
        _fp("fp_c1_3_no_plan", 3, False),
        _fp("fp_c1_128", 128, True),
        _fp("fp_no_points1", 0, True),
        _stack("stack_64_64_rows4096", 4096, 64, [64, 64]),    # narrow fused backward
        _stack("stack_20_32_rows4096", 4096, 64, [20, 32]),    # 20: a multiple of 4, not of 32
        _stack("stack_16_32_rows4096", 4096, 64, [16, 32]),    # 16: the materialised batch-norm gradient
        _stack("stack_1028_rows64", 64, 64, [1028]),           # column blocks
        _stack("dense_relu_no_bn", 4096, 64, [64], bn=False),
        _stack("conv1d_head_9", 4096, 64, [9], bn=False, conv1d=True),
        _stack("fanout_two_consumers", 4096, 64, [64, 64, 32], fanout=True),
        _sa("sa_c3_32_32_64_rows4096_no_grad", [32, 32, 64], 3, 64, no_grad=True),
    ]


# the cases each switch can change, run again with that switch off
_AFFECTED = {
    "USE_GEMM_BN_STATS": ("stack_64_64_rows4096", "sa_c3_32_32_64_rows4096"),
    "USE_BN_FINISH_IN_PRODUCER": ("stack_64_64_rows4096", "sa_c3_32_32_64_rows4096", "sa_c64_64_64_128_plan_rows32768",
                                  "msg_two_scales_hoisted", "fp_c1_3_plan_defer_last_128"),
    "USE_DGRAD_BN_STATS": ("stack_64_64_rows4096", "sa_c64_64_64_128_plan_rows4096", "msg_two_scales_hoisted"),
    "USE_BN_ON_LOAD": ("stack_64_64_rows4096", "sa_c3_32_32_64_rows4096", "fp_c1_3_plan_defer_last_128"),
    "USE_BN_GRAD_ON_LOAD": ("stack_64_64_rows4096", "stack_20_32_rows4096", "sa_c3_32_32_64_rows4096", "sa_c3_64_pooled_first"),
    "USE_POOLED_BN_REDUCE": ("sa_c3_32_32_64_rows4096", "sa_c3_64_pooled_first"),
    "USE_FUSED_BWD_NARROW": ("stack_64_64_rows4096", "sa_c3_32_32_64_rows4096"),
    "USE_SA_FIRST_LAYER_FUSED": ("sa_c3_32_32_64_rows4096", "sa_c3_32_32_64_rows2048", "sa_c3_64_pooled_first"),
    "USE_HOIST_BN_STATS": ("sa_c64_64_64_128_plan_rows32768",),
    "USE_HOISTED_TRAIN": ("sa_c64_64_64_128_plan_rows4096", "fp_c1_3_plan_defer_last_128"),
    "USE_HOISTED_MSG_TRAIN": ("msg_two_scales_hoisted", "msg_one_layer_scale_hoisted"),
}


def _cases():
    base = _base_cases()
    by_name = {c["name"]: c for c in base}
    out = list(base)
    for sw in SWITCHES:
        for name in _AFFECTED[sw]:
            out.append(dict(by_name[name], name="%s__%s_off" % (name, sw), switches={sw: False}))
    out.append(dict(by_name["stack_64_64_rows4096"], name="stack_64_64_rows4096__stats_finish_grad_on_load_off",
                    switches={"USE_GEMM_BN_STATS": False, "USE_BN_FINISH_IN_PRODUCER": False, "USE_BN_GRAD_ON_LOAD": False}))
    return out


CASES = _cases()


@contextlib.contextmanager
def _switched(mod, switches):
    """module-level A/B switches of tf_util set for one case, restored whatever happens"""
    old = {k: getattr(mod, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(mod, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(mod, k, v)


def _randomize_bn(store, seed):
    """non-trivial batch-norm parameters, moving averages and biases"""
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


def _stack_call(tfu, case, x):
    """the dense-layer cases: a conv2d chain that defers where the modules would, a conv1d head, or one layer feeding two"""
    widths, bn = case["widths"], case.get("bn", True)
    if case.get("conv1d"):
        return [tfu.conv1d(x, widths[0], 1, scope="head", activation_fn=None, bn=False, is_training=True)]
    h = x.reshape(B, case["rows"] // B, 1, case["cin"])
    conv = lambda t, i, defer=False: tfu.conv2d(t, widths[i], [1, 1], padding="VALID", stride=[1, 1], bn=bn,  # noqa: E731
                                                is_training=True, scope="conv%d" % i, bn_decay=None, defer_bn=defer)
    if case.get("fanout"):
        h = conv(h, 0)
        return [conv(h, 1), conv(h, 2)]
    for i in range(len(widths)):
        h = conv(h, i, bn and i + 1 < len(widths) and tfu.can_defer_bn(case["rows"], widths[i], widths[i + 1]))
    return [h]


def _module_call(pn2, case, dev, seed):
    """-> (inputs that require a gradient: {label: tensor}, a function of no arguments that runs the case's forward once and
    returns its output tensors).  Geometry given ahead (FPS, ball query, three_nn, scatter plans) is computed here, untraced."""
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    kind = case["kind"]
    if kind == "stack":
        x = t(rs.randn(B, case["rows"] // B, case["cin"]).astype(np.float32)).requires_grad_(True)
        return {"x": x}, lambda: _stack_call(tfu, case, x)
    if kind in ("sa", "msg"):
        c, m = case["c"], case["m"]
        xyz = t(rs.random_sample((B, N, 3)).astype(np.float32))
        pts = t(rs.randn(B, N, c).astype(np.float32))
        inputs = {}
        if c > 5:  # the level-0 module's colours carry no gradient
            inputs["points"] = pts.requires_grad_(True)
        if kind == "msg":
            radii = [0.1, 0.2]
            geo = pu.msg_geometry(xyz, m, radii, case["ks"]) if case["geo"] else None
            return inputs, lambda: [pu.pointnet_sa_module_msg(xyz, pts, m, radii, case["ks"], case["mlps"], True, None, "mod",
                                                              geometry=geo)[1]]
        geo = None
        if case["geo"] != "none":
            geo = pu.sa_geometry(xyz, m, 0.2, K)
            if case["geo"] == "plan":
                geo = (geo[0], geo[1], pu.scatter_plan(geo[1], N))
        return inputs, lambda: [pu.pointnet_sa_module(xyz, pts, npoint=m, radius=0.2, nsample=K, mlp=case["mlp"], mlp2=None,
                                                      group_all=False, is_training=True, bn_decay=None, scope="mod",
                                                      pooling=case["pooling"], geometry=geo)[1]]
    n, c1, c2, m = case["n"], case["c1"], case["c2"], 256
    xyz1 = t(rs.random_sample((B, n, 3)).astype(np.float32))
    xyz2 = xyz1[:, :m].contiguous()
    p2 = t(rs.randn(B, m, c2).astype(np.float32)).requires_grad_(True)
    inputs = {"points2": p2}
    p1 = None
    if c1:
        p1 = t(rs.randn(B, n, c1).astype(np.float32))
        if c1 > 8:  # an SA feature tensor; the level-0 colours carry no gradient
            inputs["points1"] = p1.requires_grad_(True)
    dist, idx = pn2.three_nn(xyz1, xyz2)
    nn = (dist, idx, pu.scatter_plan(idx, m, dist, weight_kind=2)) if case["plan"] else (dist, idx)

    def call():
        h = pu.pointnet_fp_module(xyz1, xyz2, p1, p2, case["mlp"], True, None, "mod", nn=nn, defer_last_bn=case["defer_last"])
        if case["defer_last"]:  # the one layer the caller promised: it applies the last batch norm while loading
            h = tfu.conv1d(h, case["defer_last"], 1, scope="fc1", bn=True, is_training=True)
        return [h]
    return inputs, call


def run_case(pn2, case, dev, seed=0):
    """-> ([(entry point, numeric args)], {label: float32 numpy array}) of one traced forward + backward"""
    tfu = pn2.util.tf_util
    store = tfu.set_default_store(tfu.VariableStore(device=dev, seed=seed))
    tfu.reset_bn_links()
    inputs, call = _module_call(pn2, case, dev, seed + 1)
    with _switched(tfu, case["switches"]):
        with torch.no_grad():
            call()  # creates the variables
        _randomize_bn(store, seed + 2)
        tfu.reset_bn_links()
        pn2._lib.lib.trace = calls = []
        try:
            if case.get("no_grad"):
                with torch.no_grad():
                    outs = call()
            else:
                outs = call()
                loss = 0.0
                for o in outs:
                    probe = torch.sin(torch.arange(o.numel(), device=dev, dtype=torch.float32) * 0.11).reshape(o.shape)
                    loss = loss + (o * probe).sum()
                loss.backward()
        finally:
            pn2._lib.lib.trace = None
    torch.cuda.synchronize()
    tensors = {"out%d" % i: o for i, o in enumerate(outs)}
    tensors.update(("grad_in/" + k, v.grad) for k, v in sorted(inputs.items()) if v.grad is not None)
    tensors.update(("grad/" + k, v.grad) for k, v in sorted(store.params.items()) if v.grad is not None)
    if store.buffers:  # the moving averages, in name order, as one tensor
        tensors["buffers"] = torch.cat([v.reshape(-1) for _, v in sorted(store.buffers.items())])
    arrays = {k: v.detach().float().contiguous().cpu().numpy() for k, v in tensors.items()}
    return [(c[0], tuple(c[1])) for c in calls], arrays


def _parse(path):
    """an output file -> {case: (the launches line, {label: hash}, {label: figure})}"""
    out, cur = {}, None
    for line in open(path):
        f = line.split()
        if f[:1] == ["case"]:
            cur = out[f[1]] = ([], {}, {})
        elif f[:1] == ["launches"]:
            cur[0].append(line.strip())
        elif f[:1] == ["tensors"]:
            for label, digest, *fig in (t.split(":") for t in f[1:]):
                cur[1][label] = digest
                cur[2][label] = float(fig[0]) if fig else 0.0
    return out


def check(parent, parent_again, head):
    """the three rules of the module docstring -> number of violations (each printed)"""
    p, pa, h = _parse(parent), _parse(parent_again), _parse(head)
    bad, loose = 0, 0
    if not (list(p) == list(pa) == list(h)):
        print("the three files do not hold the same cases")
        return 1
    for case in p:
        for other, what in ((pa, "parent_again"), (h, "head")):
            if other[case][0] != p[case][0]:
                print("%s: launch lines of %s differ from the parent's" % (case, what))
                bad += 1
        for label, digest in p[case][1].items():
            if pa[case][1][label] == digest:
                if h[case][1].get(label) != digest:
                    print("%s %s: the parent repeats this hash, the head does not" % (case, label))
                    bad += 1
                continue
            loose += 1
            own, ours = pa[case][2][label], h[case][2][label]
            print("%s %s: not repeated by the parent (%.3g); head %.3g%s" % (case, label, own, ours, "" if ours <= 2 * own else "  EXCEEDS 2x"))
            bad += ours > 2 * own
    print("%d cases, %d tensors the parent does not repeat, %d violations" % (len(p), loose, bad))
    return bad


def main(argv):
    if argv and argv[0] == "--check":
        return 1 if check(*argv[1:4]) else 0
    save = argv[argv.index("--save") + 1] if "--save" in argv else None
    against = dict(np.load(argv[argv.index("--against") + 1])) if "--against" in argv else None
    import pn2_amd as pn2
    dev = torch.device("cuda:0")
    kept = {}
    for i, case in enumerate(CASES):
        calls, arrays = run_case(pn2, case, dev, seed=200 + i)
        lines = ["%s %s" % (name, " ".join(repr(a) for a in args)) for name, args in calls]
        print("case %s" % case["name"])
        print("  launches %d args %s : %s" % (len(calls), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16],
                                            " ".join(name for name, _ in calls)))
        if "--full" in argv:
            print("".join("    %s\n" % ln for ln in lines), end="")
        tokens = []
        for label, a in arrays.items():
            tokens.append("%s:%s" % (label, hashlib.sha256(a.tobytes()).hexdigest()[:12]))
            ref = None if against is None else against.get(case["name"] + "::" + label)
            if ref is not None and ref.tobytes() != a.tobytes():
                tokens[-1] += ":%.3e" % (float(np.abs(a - ref).max()) / max(float(np.abs(ref).max()), 1e-30))
            kept[case["name"] + "::" + label] = a
        print("  tensors %s" % " ".join(tokens))
    if save:
        np.savez(save, **kept)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
