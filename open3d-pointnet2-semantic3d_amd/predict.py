"""Whole-scene prediction and dense evaluation on the device: the reference's predict.py and interpolate.py.

predict.py restores a checkpoint, samples num_samples columns per scene file, predicts them in batches of 64 (the last one
smaller), collects the sparse points with their labels and fills a sparse confusion matrix; interpolate.py votes the sparse
labels onto the dense cloud with 3-NN and evaluates against the dense ground truth.  Here:

    predictor = Predictor(checkpoint_path, num_classes, hyper_params)       # a file written by train.Trainer.save()
    points, labels = predict_scene(predictor, dataset, scene, num_samples, confusion=cm_sparse)
    dense_labels, dense_colors = label_dense(points, labels, dense_points, dense_gt_labels, confusion=cm_dense)

Every step stays on the device: the batches come from dataset.SemanticDataset.sample_batch_in_file, forward + argmax are one
captured graph per batch shape, the label pairs are counted by pn2_label_confusion (util.metric.ConfusionMatrix with device
storage) and the vote is tf_ops.tf_interpolate.interpolate_label_with_color over chunks of the dense cloud.  It is tested
on the Semantic3D flow (use_color = 1) and, through kitti_predict.PredictInterpolator, on the colourless KITTI flow.

Soft voting keeps the class probabilities where the calls above keep their argmax (include/pn2_abi.h, "Soft voting"): score rows
are integers in units of 2^-30, summed in int64, so no result depends on the order of arrival.

    scores = predictor.predict_scores(batch)                                   # (B,N,C) int32; predict_proba: float32
    labels, scores = predict_scene_tiled(predictor, dataset, scene, phases=two_grids, vote="soft")     # (n,C) int64 sums
    points, labels, scores = predict_scene(predictor, dataset, scene, num_samples, scores=True)        # (rows,C) int32
    dense_labels, dense_colors, confidence = label_dense_scores(points, scores, dense_points)
"""
import numpy as np
import torch

from . import model
from .runtime import CapturedForward
from .tf_ops.tf_interpolate import interpolate_label_with_color, interpolate_scores_with_color
from .util import metric, tf_util

SCORE_ONE = 1 << 30  # a probability of 1 as a score: score rows are integers in units of 2^-30 (include/pn2_abi.h)


def _on_device(a, dtype, device):
    """a device tensor or a numpy array -> a contiguous device tensor of `dtype`"""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device=device, dtype=dtype).contiguous()


class Predictor:
    """The reference's Predictor (predict.py:15-105), inference only.

    checkpoint_path: a file written by train.Trainer.save(); only its "variables" (parameters and moving averages by name) are
    read -- optimizer slots, step count and dropout seeds are ignored.  None keeps the fresh Xavier variables (synthetic runs).
    The variables live in the predictor's own VariableStore, created by one inference forward; the checkpoint's names and
    shapes are checked against them before anything is copied (ValueError naming up to four keys)."""

    def __init__(self, checkpoint_path, num_classes, hyper_params, device="cuda", seed=0):
        self.hp = dict(hyper_params)
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.channels = 6 if self.hp["use_color"] else 3
        self.store = tf_util.VariableStore(device=self.device, seed=seed)
        self._graphs = {}  # (B, N) -> (CapturedForward, its label stand-in): the last, smaller batch keeps the full-size graph
        self._score_graphs = {}  # (B, N) -> the same for forward + argmax + pn2_softmax_scores (predict_scores)
        self._stream = torch.cuda.Stream(device=self.device)
        # the variables: one inference forward on a column-shaped cloud (the values are not kept)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
        pc = torch.rand((1, int(self.hp["num_point"]), self.channels), generator=gen, dtype=torch.float32)
        pc[:, :, 0:2] *= 10.0
        self._run(lambda: self._forward(pc.to(self.device), None))
        if checkpoint_path is not None:
            state = torch.load(checkpoint_path, weights_only=True, map_location="cpu")
            self._load_variables(state["variables"])

    def _load_variables(self, variables):
        have = {k: v for k, v in list(self.store.params.items()) + list(self.store.buffers.items())}
        # names the model does not know first, then the ones the checkpoint lacks: up to four in all
        diff = sorted(set(variables) - set(have)) + sorted(set(have) - set(variables))
        if diff:
            raise ValueError("the checkpoint's variables differ from this model's: %s%s"
                             % (", ".join(diff[:4]), " ..." if len(diff) > 4 else ""))
        bad = [k for k, v in have.items() if tuple(variables[k].shape) != tuple(v.shape)]
        if bad:
            raise ValueError("the checkpoint holds other shapes than this model (num_classes, hyper_params?): %s%s" % (
                ", ".join("%s %s, here %s" % (k, tuple(variables[k].shape), tuple(have[k].shape)) for k in bad[:4]),
                " ..." if len(bad) > 4 else ""))

        def copy():
            with torch.no_grad():
                for k, v in have.items():
                    v.copy_(variables[k].to(self.device))
        self._run(copy)
        self.store.train_epoch += 1  # the folded inference weights are made again from the loaded values

    def _run(self, fn):
        """fn() on the predictor's stream (graph replays stay off the null stream, as in train.Trainer), ordered after the
        caller's work so far and before its later work"""
        previous = tf_util._default_store  # the program's own default store is put back: eager model calls after a predict()
        tf_util.set_default_store(self.store)  # do not land in the predictor's
        try:
            caller = torch.cuda.current_stream(self.device)
            self._stream.wait_stream(caller)
            with torch.cuda.stream(self._stream), torch.no_grad():
                out = fn()
            caller.wait_stream(self._stream)
        finally:
            tf_util.set_default_store(previous)
        return out

    def _forward(self, pc, labels):
        """logits, and with `labels` (the int32 stand-in pn2_confusion_update asks for; it counts nothing here) their argmax
        with np.argmax semantics -- the kernel's `pred` output, launched inside the graph"""
        logits, _ = model.get_model(pc, False, self.num_classes, self.hp)
        if labels is None:
            return logits
        pred = torch.empty(tuple(logits.shape[:2]), dtype=torch.int32, device=logits.device)
        metric.confusion_update(logits, labels, pred=pred)
        return pred

    def predict(self, batch_data):
        """batch_data (B,N,6) float32 ((B,N,3) without colour), a device tensor or a numpy array -> (B,N) int32 labels on the
        device (predict.py:65-91).  The first call for a (B, N) captures forward + argmax into one graph (that call
        synchronises); later calls replay it.  The result is a fresh tensor: later calls do not overwrite it."""
        shape = tuple(batch_data.shape)
        if len(shape) != 3 or shape[2] != self.channels:
            raise ValueError("batch_data must be (batch_size, num_point, %d) with use_color = %d, got %s"
                             % (self.channels, int(bool(self.hp["use_color"])), shape))
        x = _on_device(batch_data, torch.float32, self.device)

        def run():
            ent = self._graphs.get(shape[:2])
            if ent is None:
                labels = torch.zeros(shape[0] * shape[1], dtype=torch.int32, device=self.device)
                ent = (CapturedForward(lambda pc: self._forward(pc, labels), x), labels)
                self._graphs[shape[:2]] = ent
            return ent[0](x).clone()

        out = self._run(run)
        out.record_stream(torch.cuda.current_stream(self.device))
        return out

    def _forward_scores(self, pc, labels):
        """the argmax of _forward and, from the same logits, their score rows (pn2_softmax_scores), both inside the graph"""
        from ._lib import launch, ptr
        logits = self._forward(pc, None).contiguous()
        pred = torch.empty(tuple(logits.shape[:2]), dtype=torch.int32, device=logits.device)
        metric.confusion_update(logits, labels, pred=pred)
        q = torch.empty(tuple(logits.shape), dtype=torch.int32, device=logits.device)
        launch("pn2_softmax_scores", logits, logits.shape[0] * logits.shape[1], logits.shape[2], ptr(logits), ptr(q), None)
        return pred, q

    def predict_labels_and_scores(self, batch_data):
        """-> predict's (B,N) int32 labels and predict_scores' (B,N,C) int32 score rows from ONE forward pass: forward, argmax
        and pn2_softmax_scores are one captured graph per (B, N), kept beside predict's label graph.  Fresh tensors."""
        shape = tuple(batch_data.shape)
        if len(shape) != 3 or shape[2] != self.channels:
            raise ValueError("batch_data must be (batch_size, num_point, %d) with use_color = %d, got %s"
                             % (self.channels, int(bool(self.hp["use_color"])), shape))
        x = _on_device(batch_data, torch.float32, self.device)

        def run():
            ent = self._score_graphs.get(shape[:2])
            if ent is None:
                labels = torch.zeros(shape[0] * shape[1], dtype=torch.int32, device=self.device)
                ent = (CapturedForward(lambda pc: self._forward_scores(pc, labels), x), labels)
                self._score_graphs[shape[:2]] = ent
            pred, q = ent[0](x)
            return pred.clone(), q.clone()

        pred, q = self._run(run)
        for t in (pred, q):
            t.record_stream(torch.cuda.current_stream(self.device))
        return pred, q

    def predict_scores(self, batch_data):
        """batch_data as predict takes it -> (B,N,C) int32 score rows on the device: q = rint(softmax(logits) * 2^30), the
        softmax in float64 (pn2_softmax_scores); a row whose logits hold a NaN or an infinite maximum is all zero.  The first
        call for a (B, N) captures forward + softmax into one graph (that call synchronises); later calls replay it.  The result
        is a fresh tensor."""
        return self.predict_labels_and_scores(batch_data)[1]

    def predict_proba(self, batch_data):
        """-> (B,N,C) float32 class probabilities: predict_scores * 2^-30"""
        return self.predict_scores(batch_data).to(torch.float32) * (1.0 / SCORE_ONE)

    def interpolate_labels(self, sparse_points, sparse_labels, dense_points):
        """predict.py:93-105: the 3-NN majority vote of the sparse labels onto dense_points -> dense_labels (nd,) int32,
        dense_colors (nd,3) uint8"""
        sp = _on_device(sparse_points, torch.float32, self.device)
        sl = _on_device(sparse_labels, torch.int32, self.device)
        return interpolate_label_with_color(sp, sl, _on_device(dense_points, torch.float32, self.device), 3)


def predict_scene(predictor, dataset, scene, num_samples, batch_size=64, confusion=None, scores=False):
    """predict.py:152-188 for one scene of a dataset.SemanticDataset: ceil(num_samples / batch_size) batches of columns of
    that scene (the last one smaller), each sample_batch_in_file -> predict.  -> sparse_points (num_samples * N, 3) float32 (the
    raw points; the reference passes them through a float32 .pcd) and sparse_labels (num_samples * N,) int32, on the device.
    confusion (util.metric.ConfusionMatrix): counts each batch's (ground truth, prediction) pairs.  Nothing in the loop waits
    for the device, apart from the capture of a batch size the predictor has not seen.  The worst sample status of ALL the
    scene's batches is kept on the device and left in dataset.last_status (one element), so one dataset.check_last() after the
    call tells whether any sample of the scene was rejected (zero-filled) -- not only one of the last batch.
    scores=True: also returns the (num_samples * N, C) int32 score rows of the collected points (Predictor.predict_scores), from
    the same forward pass as the labels; the labels are the ones scores=False gives."""
    num_samples, batch_size = int(num_samples), int(batch_size)
    if num_samples <= 0 or batch_size <= 0:
        raise ValueError("num_samples and batch_size must be positive")
    n = dataset.num_points_per_sample
    points = torch.empty((num_samples * n, 3), dtype=torch.float32, device=predictor.device)
    labels = torch.empty((num_samples * n,), dtype=torch.int32, device=predictor.device)
    worst = torch.zeros(1, dtype=torch.int32, device=predictor.device)
    rows = torch.empty((num_samples * n, predictor.num_classes), dtype=torch.int32, device=predictor.device) if scores else None
    done = 0
    while done < num_samples:
        b = min(batch_size, num_samples - done)
        data, raw, gt = dataset.sample_batch_in_file(scene, b)
        worst = torch.maximum(worst, dataset.last_status.max())
        if scores:
            pred, q = predictor.predict_labels_and_scores(data)
            rows[done * n:(done + b) * n].copy_(q.reshape(-1, predictor.num_classes))
        else:
            pred = predictor.predict(data)
        points[done * n:(done + b) * n].copy_(raw.reshape(-1, 3))  # float64 -> float32
        labels[done * n:(done + b) * n].copy_(pred.reshape(-1))
        if confusion is not None:
            confusion.increment_from_list(gt.reshape(-1), pred.reshape(-1))
        done += b
    dataset.last_status = worst
    return (points, labels, rows) if scores else (points, labels)


def label_dense(sparse_points, sparse_labels, dense_points, dense_gt_labels=None, confusion=None, knn=3, chunk=1 << 24):
    """interpolate.py:105-124: every dense point takes the majority label of its knn nearest sparse points.  sparse_points
    (ns,3) / sparse_labels (ns,): device tensors or numpy arrays; dense_points (nd,3): a device tensor, or a numpy array that
    is uploaded chunk by chunk (`chunk` dense points per interpolate_label_with_color call: a dense point's vote does not
    depend on the others, so neither does the result on `chunk`).  -> dense_labels (nd,) int32, dense_colors (nd,3) uint8 on
    the device.  With dense_gt_labels (nd,) and confusion (util.metric.ConfusionMatrix) every chunk's (ground truth, label)
    pairs are counted."""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    dev = sparse_points.device if torch.is_tensor(sparse_points) else (
        dense_points.device if torch.is_tensor(dense_points) else torch.device("cuda", torch.cuda.current_device()))
    sp = _on_device(sparse_points, torch.float32, dev)
    sl = _on_device(sparse_labels, torch.int32, dev)
    nd = int(dense_points.shape[0])
    if tuple(dense_points.shape) != (nd, 3):
        raise ValueError("dense_points must be: (num_dense_points, 3)")
    count = dense_gt_labels is not None and confusion is not None
    if count and int(dense_gt_labels.shape[0]) != nd:
        raise ValueError("dense_gt_labels and dense_points differ in length")
    labels = torch.empty((nd,), dtype=torch.int32, device=dev)
    colors = torch.empty((nd, 3), dtype=torch.uint8, device=dev)
    for lo in range(0, nd, chunk):
        hi = min(nd, lo + chunk)
        lab, col = interpolate_label_with_color(sp, sl, _on_device(dense_points[lo:hi], torch.float32, dev), knn)
        labels[lo:hi].copy_(lab)
        colors[lo:hi].copy_(col)
        if count:
            gt = dense_gt_labels[lo:hi]
            wide = (gt.dtype == torch.int64) if torch.is_tensor(gt) else (np.asarray(gt).dtype.itemsize > 4)
            # int64 ground truth stays int64: a value beyond int32 must be dropped, not wrapped into a class
            confusion.increment_from_list(_on_device(gt, torch.int64 if wide else torch.int32, dev), labels[lo:hi])
    return labels, colors


def label_dense_scores(sparse_points, sparse_scores, dense_points, dense_gt_labels=None, confusion=None, knn=3, chunk=1 << 24):
    """label_dense on scores: every dense point takes the class whose scores, summed over its knn nearest sparse points, are the
    largest (interpolate_scores_with_color: int64 sums, the first maximal class).  sparse_scores (ns,C): int64 accumulated rows
    (predict_scene_tiled(vote="soft")) or int32 score rows (predict_scene(scores=True)), widened here.  Chunked and counted as
    label_dense is.  -> dense_labels (nd,) int32, dense_colors (nd,3) uint8, dense_confidence (nd,) float32 on the device."""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    dev = sparse_points.device if torch.is_tensor(sparse_points) else (
        dense_points.device if torch.is_tensor(dense_points) else torch.device("cuda", torch.cuda.current_device()))
    sp = _on_device(sparse_points, torch.float32, dev)
    ss = _on_device(sparse_scores, torch.int64, dev)
    nd = int(dense_points.shape[0])
    if tuple(dense_points.shape) != (nd, 3):
        raise ValueError("dense_points must be: (num_dense_points, 3)")
    count = dense_gt_labels is not None and confusion is not None
    if count and int(dense_gt_labels.shape[0]) != nd:
        raise ValueError("dense_gt_labels and dense_points differ in length")
    labels = torch.empty((nd,), dtype=torch.int32, device=dev)
    colors = torch.empty((nd, 3), dtype=torch.uint8, device=dev)
    confidence = torch.empty((nd,), dtype=torch.float32, device=dev)
    for lo in range(0, nd, chunk):
        hi = min(nd, lo + chunk)
        lab, col, conf = interpolate_scores_with_color(sp, ss, _on_device(dense_points[lo:hi], torch.float32, dev), knn)
        labels[lo:hi].copy_(lab)
        colors[lo:hi].copy_(col)
        confidence[lo:hi].copy_(conf)
        if count:
            gt = dense_gt_labels[lo:hi]
            wide = (gt.dtype == torch.int64) if torch.is_tensor(gt) else (np.asarray(gt).dtype.itemsize > 4)
            confusion.increment_from_list(_on_device(gt, torch.int64 if wide else torch.int32, dev), labels[lo:hi])
    return labels, colors, confidence


def predict_scene_tiled(predictor, dataset, scene, batch_size=64, phases=((0.0, 0.0),), min_points=1, confusion=None, vote="hard"):
    """A label for every point of scene `scene` of a dataset.SemanticDataset: the whole-scene evaluation of PointNet++'s
    ScanNet code on this network's columns, where predict_scene leaves coverage to its random draws.  Per phase (a grid shift
    in metres, >= 0) the scene is cut into box_size_x x box_size_y columns, every column with at least min_points points into
    as many num_point-sized samples as it takes to use each of its points once (dataset.tile_cover: pn2_tile_plan); the samples
    are predicted in batches of exactly batch_size (the last one padded with a repeated sample that does not vote, so the
    predictor captures ONE graph), and every prediction is added to its point's row of `votes` (pn2_tile_vote).  The label of a
    point is the first class with the most votes over all phases; a point nobody voted for (a column below min_points in every
    phase) gets 0, "unlabeled".  phases=((0, 0), (box_size_x / 2, box_size_y / 2)) is the usual overlapping cover.
    -> labels (n,) int32, votes (n, num_classes) int32, on the device, aligned with dataset.scene_points[scene] (the scene
    sorted by x): with ingest="device", keep_perm=True, labels[i] belongs to input row dataset.scene_perm[scene][i], so
    out = torch.empty_like(labels); out[dataset.scene_perm[scene].long()] = labels is in input order.
    confusion (util.metric.ConfusionMatrix): counts the (scene label, final label) pair of every point, once.
    vote="soft": the class probabilities vote instead of their argmax.  Every live row adds its score row (Predictor.predict_scores:
    integers in units of 2^-30) to its point's row of `scores` (pn2_tile_vote_scores, int64 adds), and the label is the first
    class with the largest sum (pn2_score_labels): two grids that disagree are settled by how sure each was, not by the class
    number.  -> labels (n,) int32, scores (n, num_classes) int64.  The same cover, the same single graph shape, the same reads.
    Per phase one 32-byte read-back (the plan's header: how many batches to launch); the batch loop does not wait for the
    device, apart from the capture of a batch shape the predictor has not seen."""
    from ._lib import launch, ptr
    batch_size = int(batch_size)
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    if vote not in ("hard", "soft"):
        raise ValueError("vote must be \"hard\" or \"soft\"")
    soft = vote == "soft"
    phases = [(float(p[0]), float(p[1])) for p in phases]
    if not phases:
        raise ValueError("phases: at least one (phase_x, phase_y)")
    dev, c, npts = predictor.device, predictor.num_classes, dataset.num_points_per_sample
    n = int(dataset.scene_counts[int(scene)])
    votes = torch.zeros((n, c), dtype=torch.int64 if soft else torch.int32, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    for phase in phases:
        cover = dataset.tile_cover(scene, phase, min_points)
        for q0 in range(0, cover.num_samples, batch_size):
            data, sel, live = cover.batch(q0, batch_size)
            if soft:
                q = predictor.predict_scores(data)
                launch("pn2_tile_vote_scores", dev, batch_size, npts, c, ptr(sel), ptr(live), ptr(q), ptr(votes), None)
            else:
                pred = predictor.predict(data)
                launch("pn2_tile_vote", dev, batch_size, npts, c, ptr(sel), ptr(live), ptr(pred), ptr(votes), None)
    if soft:
        launch("pn2_score_labels", dev, n, c, ptr(votes), ptr(labels), None)
    else:
        launch("pn2_tile_labels", dev, n, c, ptr(votes), ptr(labels))
    if confusion is not None:
        gt = dataset.scene_labels[int(scene)]
        confusion.increment_from_list(_on_device(gt, torch.int32, dev), labels)
    return labels, votes
