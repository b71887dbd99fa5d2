"""What the tiled cover of a scene costs ("Tiled whole-scene prediction"): one JSON line with, on the
synthetic training store of examples/train_semantic3d.py (2.8 M points in 3 scenes), N = 8192, B = 64, per scene
  plan    pn2_tile_plan (one call: the scene's tiles, order and table of samples),
  gather  pn2_tile_gather over every batch of the pass,
  vote    pn2_tile_vote over every batch of the pass,
each against a restatement of the same step in torch ops, run in the same call on the same inputs (and checked to give the same
result first): the library is never its own yardstick.  Then predict.predict_scene_tiled per scene, one grid and two, with
fresh weights (the time does not depend on them).
Every figure is the median of 5 regions in this process, the device synchronised on both sides of each.
usage: python tools/tiled_predict_cost.py [--skip-predict]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import pn2_amd as pn2  # noqa: E402
import train_semantic3d as ex  # noqa: E402

launch, ptr, u64_array = pn2._lib.launch, pn2._lib.ptr, pn2._lib.u64_array

N, B, C = 8192, 64, 9
BOX = 10.0


def wall_ms(fn, reps=5):
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(v)), 3), [round(x, 3) for x in v]


# ---- the three steps in torch ops ------------------------------------------------------------------------------------------
def torch_plan(points, phase):
    """rules 1-3: -> order (n,) int64, table (n_samples,4) int64"""
    n = points.shape[0]
    ox, oy = points[0, 0] - phase[0], points[:, 1].min() - phase[1]
    i = torch.floor((points[:, 0] - ox) / BOX).long()
    j = torch.floor((points[:, 1] - oy) / BOX).long()
    key = (i << 32) | j
    skey, order = torch.sort(key, stable=True)
    _, m = torch.unique_consecutive(skey, return_counts=True)
    a = torch.cumsum(m, 0) - m
    S = (m + N - 1) // N
    tile = torch.repeat_interleave(torch.arange(len(m), device=points.device), S)
    first = torch.cumsum(S, 0) - S
    s = torch.arange(len(tile), device=points.device) - first[tile]
    return order, torch.stack([a[tile], m[tile], s, S[tile]], 1)


def torch_gather(points, colors, order, table, q0):
    ns = table.shape[0]
    q = torch.arange(q0, q0 + B, device=points.device)
    rows = table[torch.clamp(q, max=ns - 1)]
    a, m, s, S = rows[:, 0:1], rows[:, 1:2], rows[:, 2:3], rows[:, 3:4]
    c = (m - s + S - 1) // S
    k = torch.arange(N, device=points.device)[None, :]
    sel = order[a + s + (k % c) * S]
    p = points[sel]
    shift = p.min(1, keepdim=True)[0]
    shift[:, :, 0] += BOX / 2
    shift[:, :, 1] += BOX / 2
    data = torch.cat([(p - shift).float(), colors[sel]], 2)
    live = torch.where(q < ns, c[:, 0], torch.zeros_like(q))
    return data, sel.int(), live.int()


def torch_vote(votes, sel, live, pred):
    k = torch.arange(N, device=sel.device)[None, :]
    ok = (k < live[:, None]) & (pred >= 0) & (pred < C)
    flat = (sel.long() * C + pred.long())[ok]
    votes.view(-1).index_add_(0, flat, torch.ones_like(flat, dtype=torch.int32))


# ---- the library's ----------------------------------------------------------------------------------------------------------
def lib_plan(dev, points, phase, order, table, header, ws):
    n = points.shape[0]
    launch("pn2_tile_plan", dev, n, ptr(points), BOX, BOX, phase[0], phase[1], N, 1, table.shape[0], ptr(order), ptr(table),
           ptr(header), ptr(ws), ws.numel())


def scene_cost(dev, ds, k, phase):
    out = {}
    d = ds._upload(1)
    v = ds._scene_view(d, k)
    points, colors = v["points"], v["colors"]
    n = points.shape[0]
    nbytes = u64_array([0])
    launch("pn2_tile_plan_workspace_size", dev, n, nbytes, stream=False)
    ws = torch.empty((int(nbytes[0]) + 256,), dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) % 256:]
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    table = torch.empty((n // N + 4096, 4), dtype=torch.int32, device=dev)
    header = torch.empty((8,), dtype=torch.int32, device=dev)
    lib_plan(dev, points, phase, order, table, header, ws)
    h = header.cpu().tolist()
    assert h[3] == 0, h
    ns = h[1]
    t_order, t_table = torch_plan(points, phase)
    assert torch.equal(order.long(), t_order) and torch.equal(table[:ns].long(), t_table), "the torch restatement disagrees (plan)"
    out.update(points=n, tiles=h[0], samples=ns, batches=(ns + B - 1) // B, workspace_mb=round(int(nbytes[0]) / 2 ** 20, 1))
    out["plan_ms"], out["plan_runs"] = wall_ms(lambda: lib_plan(dev, points, phase, order, table, header, ws))
    out["plan_torch_ms"], out["plan_torch_runs"] = wall_ms(lambda: torch_plan(points, phase))

    data = torch.empty((B, N, 6), dtype=torch.float32, device=dev)
    sel = torch.empty((B, N), dtype=torch.int32, device=dev)
    live = torch.empty((B,), dtype=torch.int32, device=dev)

    def lib_gather(q0):
        launch("pn2_tile_gather", dev, B, N, q0, 1, ptr(points), ptr(colors), ptr(order), ptr(table), ptr(header), BOX, BOX,
               ptr(data), ptr(sel), ptr(live))
    for q0 in range(0, ns, B):
        lib_gather(q0)
        t_data, t_sel, t_live = torch_gather(points, colors, t_order, t_table, q0)
        assert torch.equal(sel, t_sel) and torch.equal(live, t_live), "the torch restatement disagrees (gather)"
        assert torch.equal(data.view(torch.int32), t_data.view(torch.int32)), "the torch restatement disagrees (gather data)"
    out["gather_ms"], out["gather_runs"] = wall_ms(lambda: [lib_gather(q0) for q0 in range(0, ns, B)])
    out["gather_torch_ms"], out["gather_torch_runs"] = wall_ms(
        lambda: [torch_gather(points, colors, t_order, t_table, q0) for q0 in range(0, ns, B)])

    gen = torch.Generator(device="cpu").manual_seed(k)
    batches = []
    for q0 in range(0, ns, B):
        lib_gather(q0)
        batches.append((sel.clone(), live.clone(), torch.randint(0, C, (B, N), generator=gen, dtype=torch.int32).to(dev)))
    votes, t_votes = torch.zeros((n, C), dtype=torch.int32, device=dev), torch.zeros((n, C), dtype=torch.int32, device=dev)

    def lib_vote():
        for s_, l_, p_ in batches:
            launch("pn2_tile_vote", dev, B, N, C, ptr(s_), ptr(l_), ptr(p_), ptr(votes), None)

    def t_vote():
        for s_, l_, p_ in batches:
            torch_vote(t_votes, s_, l_, p_)
    lib_vote()
    t_vote()
    assert torch.equal(votes, t_votes) and bool((votes.sum(1) == 1).all()), "the torch restatement disagrees (vote)"
    out["vote_ms"], out["vote_runs"] = wall_ms(lib_vote)
    out["vote_torch_ms"], out["vote_torch_runs"] = wall_ms(t_vote)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-predict", action="store_true", help="the three steps only, without the network")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    scenes = [ex.synthetic_scene(*ex.SYNTHETIC[k]) + (k,) for k in ex.SYNTHETIC_SPLITS["train"]]
    ds = pn2.dataset.SemanticDataset(N, "train", True, BOX, BOX, "", device=dev, seed=0, scenes=scenes, ingest="device")
    out = {"N": N, "B": B, "scenes": {}}
    for k, name in enumerate(ds.scene_names):
        scene_cost(dev, ds, k, (0.0, 0.0))  # warm-up: allocator, the sort's first call
        out["scenes"][name] = scene_cost(dev, ds, k, (0.0, 0.0))
    if not args.skip_predict:
        hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
        hp.update(num_point=N, use_color=1)
        predictor = pn2.predict.Predictor(None, C, hp, device=dev)
        two = ((0.0, 0.0), (BOX / 2, BOX / 2))
        pn2.predict.predict_scene_tiled(predictor, ds, 0, B)  # the capture
        for k, name in enumerate(ds.scene_names):
            o = out["scenes"][name]
            o["predict_1_grid_ms"], o["predict_1_grid_runs"] = wall_ms(lambda: pn2.predict.predict_scene_tiled(predictor, ds, k, B))
            o["predict_2_grids_ms"], o["predict_2_grids_runs"] = wall_ms(
                lambda: pn2.predict.predict_scene_tiled(predictor, ds, k, B, phases=two))
        out["graphs"] = len(predictor._graphs)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
