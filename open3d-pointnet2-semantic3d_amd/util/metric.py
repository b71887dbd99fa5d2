"""Confusion matrix, IoU and accuracy of the reference's util/metric.py, with the counting on the device.

The reference builds a `ConfusionMatrix` per epoch (train.py:199-331, predict.py) and fills it with one Python `increment`
per point after reading the logits back to the host.  Here the same class keeps its counts either in a numpy array (the
reference's behaviour, `device=None`) or in a device int64 tensor (`device="cuda"`): `increment_from_logits` then runs
pn2_confusion_update -- argmax and counting in one launch, no host synchronisation -- so it can sit inside a captured
training step.  Reading `confusion_matrix` or any `get_*` is the only synchronisation.
`increment_from_list` on device label tensors (predict.py, interpolate.py) runs pn2_label_confusion: the same counting from two
label arrays, without temporaries.

Semantic3D convention (the reference's): ground-truth label 0 ("unlabeled") is ignored by the IoU and the accuracy.
"""
from pprint import pprint

import numpy as np
import torch

# labels_names of the reference's dataset/semantic_dataset.py (the Semantic3D classes; index = label)
SEMANTIC3D_LABELS_NAMES = [
    "unlabeled",
    "man-made terrain",
    "natural terrain",
    "high vegetation",
    "low vegetation",
    "buildings",
    "hard scape",
    "scanning artifact",
    "cars",
]

MAX_CLASSES = 64  # pn2_confusion_update, pn2_label_confusion (= the cross-entropy kernel's limit)


def _flat_labels(labels):
    if labels.dtype not in (torch.int32, torch.int64):
        labels = labels.long()
    return labels.reshape(-1).contiguous()


def confusion_update(logits, labels, confusion=None, invalid=None, pred=None, loss=None, loss_acc=None):
    """One pn2_confusion_update launch on the current stream.  logits (..., C) float32 on the device, labels (...) integer;
    confusion: int64 tensor of C*C elements (added to), invalid: int64 tensor of one element (added to: labels outside
    [0, C)), pred: int32 tensor of rows elements (written: the argmax), loss / loss_acc: device f32 scalar and float64 [sum,
    count] (added to).  Every output is optional; at least one must be given."""
    from .._lib import launch, ptr, require_cuda
    require_cuda(logits, labels)
    c = int(logits.shape[-1])
    z = logits.detach().reshape(-1, c)
    if z.dtype != torch.float32 or not z.is_contiguous():
        z = z.float().contiguous()
    lab = _flat_labels(labels)
    rows = z.shape[0]
    if lab.numel() != rows:
        raise ValueError("labels hold %d elements for %d rows of logits" % (lab.numel(), rows))
    for name, t, n, dt in (("confusion", confusion, c * c, torch.int64), ("invalid", invalid, 1, torch.int64),
                           ("pred", pred, rows, torch.int32), ("loss", loss, 1, torch.float32),
                           ("loss_acc", loss_acc, 2, torch.float64)):
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != z.device):
            raise ValueError("%s: a contiguous %s tensor of %d elements on %s expected" % (name, dt, n, z.device))
    launch("pn2_confusion_update", z, rows, c, ptr(z), ptr(lab), int(lab.dtype == torch.int64), ptr(pred), ptr(confusion), ptr(invalid),
           ptr(loss), ptr(loss_acc))


def label_confusion(gt_labels, pd_labels, confusion, dropped=None):
    """One pn2_label_confusion launch on the current stream: confusion (C*C int64, added to)[gt * C + pd] += 1 for every pair
    of the two flat, contiguous device label tensors (both int32 or both int64) with both labels in [0, C); the other pairs
    are left out and counted in dropped (int64 tensor of one element, added to) when given."""
    from .._lib import launch, ptr, require_cuda
    require_cuda(gt_labels, pd_labels, confusion, dropped)
    n = gt_labels.numel()
    if gt_labels.dtype != pd_labels.dtype or gt_labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("gt_labels and pd_labels: both int32 or both int64")
    if pd_labels.numel() != n or not (gt_labels.is_contiguous() and pd_labels.is_contiguous()):
        raise ValueError("gt_labels and pd_labels: contiguous and of one length")
    c = int(round(confusion.numel() ** 0.5))
    for name, t, m in (("confusion", confusion, c * c), ("dropped", dropped, 1)):
        if t is not None and (t.dtype != torch.int64 or t.numel() != m or not t.is_contiguous() or t.device != gt_labels.device):
            raise ValueError("%s: a contiguous int64 tensor of %d elements on %s expected" % (name, m, gt_labels.device))
    launch("pn2_label_confusion", gt_labels, n, c, ptr(gt_labels), ptr(pd_labels), int(gt_labels.dtype == torch.int64),
           ptr(confusion), ptr(dropped))


class ConfusionMatrix:
    """util/metric.py's ConfusionMatrix: rows = ground truth, columns = prediction.

    device=None: counts in a numpy int64 array (`confusion_matrix`), exactly the reference's class.
    device="cuda[:i]": counts in a device int64 tensor; `increment_from_logits` and `increment_from_list` on device tensors
    never synchronise, `reset()` zeroes the counts on the current stream, and reading `confusion_matrix`, `num_invalid` or
    any `get_*` copies them to the host (the one synchronisation)."""

    def __init__(self, num_classes, device=None):
        """label must be {0, 1, 2, ..., num_classes - 1}"""
        self.num_classes = int(num_classes)
        self.valid_labels = set(range(self.num_classes))
        self.device = None if device is None else torch.device(device)
        c2 = self.num_classes * self.num_classes
        if self.device is None:
            self._cm = np.zeros((self.num_classes, self.num_classes), dtype=np.int64)
            self._invalid = 0
            self.counts = None
        else:
            # [matrix (C*C) | labels outside [0, C) | dump slot of increment_from_list] in ONE tensor: one read-back
            self.counts = torch.zeros(c2 + 2, dtype=torch.int64, device=self.device)

    # ---- storage -------------------------------------------------------------------------------------------------
    @property
    def on_device(self):
        return self.device is not None

    @property
    def matrix_tensor(self):
        """the device counts as a (C, C) view (device storage only): what pn2_confusion_update adds into"""
        c = self.num_classes
        return self.counts[:c * c].view(c, c)

    @property
    def invalid_tensor(self):
        c = self.num_classes
        return self.counts[c * c:c * c + 1]

    @property
    def confusion_matrix(self):
        """(C, C) numpy int64.  Host storage: the array itself (mutable, as in the reference); device storage: a copy."""
        if self.device is None:
            return self._cm
        return self.matrix_tensor.cpu().numpy()

    @confusion_matrix.setter
    def confusion_matrix(self, value):
        value = np.asarray(value, dtype=np.int64).reshape(self.num_classes, self.num_classes)
        if self.device is None:
            self._cm = value.copy()
        else:
            self.matrix_tensor.copy_(torch.from_numpy(value))

    @property
    def num_invalid(self):
        """how many labels outside [0, num_classes) increment_from_logits has met (they are not in the matrix)"""
        if self.device is None:
            return int(self._invalid)
        return int(self.invalid_tensor.item())

    def reset(self):
        """zero the counts (device storage: a fill on the current stream, no synchronisation)"""
        if self.device is None:
            self._cm[...] = 0
            self._invalid = 0
        else:
            self.counts.zero_()

    # ---- counting ------------------------------------------------------------------------------------------------
    def increment(self, gt_label, pd_label):
        if gt_label not in self.valid_labels:
            raise ValueError("Invalid value for gt_label")
        if pd_label not in self.valid_labels:
            raise ValueError("Invalid value for pd_label")
        if self.device is None:
            self._cm[gt_label][pd_label] += 1
        else:
            self.counts[int(gt_label) * self.num_classes + int(pd_label)] += 1

    def increment_from_list(self, gt_labels, pd_labels):
        """add the pairs (gt, pd); pairs with a label outside [0, num_classes) are dropped (sklearn's confusion_matrix with
        labels=range(num_classes), as the reference calls it).  Device storage and device tensors: stays on the device."""
        c = self.num_classes
        if self.device is not None and torch.is_tensor(gt_labels) and gt_labels.is_cuda:
            if c <= MAX_CLASSES:
                # pn2_label_confusion: int32 / int64 contiguous inputs go in as they are, anything else is cast once
                gt, pd = gt_labels.reshape(-1), torch.as_tensor(pd_labels, device=gt_labels.device).reshape(-1)
                if gt.numel() != pd.numel():
                    raise ValueError("gt_labels and pd_labels differ in length")
                if gt.dtype != pd.dtype or gt.dtype not in (torch.int32, torch.int64):
                    gt, pd = gt.long(), pd.long()
                gt, pd = gt.contiguous(), pd.contiguous()
                if gt.numel():
                    label_confusion(gt, pd, self.counts[:c * c])
                return
            # above the kernel's class limit: torch
            gt = gt_labels.reshape(-1).long()
            pd = torch.as_tensor(pd_labels, device=gt.device).reshape(-1).long()
            if gt.numel() != pd.numel():
                raise ValueError("gt_labels and pd_labels differ in length")
            ok = (gt >= 0) & (gt < c) & (pd >= 0) & (pd < c)
            idx = torch.where(ok, gt * c + pd, torch.full_like(gt, c * c + 1))  # out-of-range pairs land in the dump slot
            self.counts.scatter_add_(0, idx, torch.ones_like(idx))
            self.counts[c * c + 1:].zero_()
            return
        gt = np.asarray(gt_labels.cpu() if torch.is_tensor(gt_labels) else gt_labels).reshape(-1).astype(np.int64)
        pd = np.asarray(pd_labels.cpu() if torch.is_tensor(pd_labels) else pd_labels).reshape(-1).astype(np.int64)
        if gt.shape != pd.shape:
            raise ValueError("gt_labels and pd_labels differ in length")
        ok = (gt >= 0) & (gt < c) & (pd >= 0) & (pd < c)
        inc = np.bincount(gt[ok] * c + pd[ok], minlength=c * c).reshape(c, c).astype(np.int64)
        if self.device is None:
            self._cm += inc
        else:
            self.matrix_tensor.add_(torch.from_numpy(inc).to(self.device))

    def increment_from_logits(self, logits, labels, return_pred=False):
        """argmax over the last axis of `logits` (..., C) (np.argmax semantics: first maximum, NaN counts as the maximum)
        against `labels` (...), on the device in one launch.  Labels outside [0, C) are counted in num_invalid instead.
        Device storage: no synchronisation.  Host storage: the batch is counted on the device and added to the array
        (one synchronisation).  return_pred: also -> the argmax, int32 of labels' shape, on the device."""
        if int(logits.shape[-1]) != self.num_classes:
            raise ValueError("logits have %d classes, the matrix %d" % (int(logits.shape[-1]), self.num_classes))
        pred = None
        if return_pred:
            pred = torch.empty(tuple(labels.shape), dtype=torch.int32, device=logits.device)
        if self.device is not None:
            confusion_update(logits, labels, confusion=self.matrix_tensor, invalid=self.invalid_tensor, pred=pred)
        else:
            c = self.num_classes
            tmp = torch.zeros(c * c + 1, dtype=torch.int64, device=logits.device)
            confusion_update(logits, labels, confusion=tmp[:c * c], invalid=tmp[c * c:], pred=pred)
            host = tmp.cpu().numpy()
            self._cm += host[:c * c].reshape(c, c)
            self._invalid += int(host[c * c])
        return pred if return_pred else None

    def all_reduce_(self, group=None):
        """sum the counts over the ranks of `group` (torch.distributed; a no-op without a process group or with one rank).
        Host storage goes through a tensor on the backend's device; device storage is reduced in place."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if self.device is not None:
            dist.all_reduce(self.counts, group=group)
            return self
        dev = torch.device("cpu")
        if dist.get_backend(group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        t = torch.from_numpy(np.concatenate([self._cm.reshape(-1), [self._invalid]]).astype(np.int64)).to(dev)
        dist.all_reduce(t, group=group)
        host = t.cpu().numpy()
        c = self.num_classes
        self._cm[...] = host[:c * c].reshape(c, c)
        self._invalid = int(host[c * c])
        return self

    # ---- metrics (util/metric.py) --------------------------------------------------------------------------------
    def get_per_class_ious(self):
        """IoU of the classes 1 .. C-1 (label 0 ignored: Semantic3D).  A list of num_classes - 1 floats."""
        cm = self.confusion_matrix
        # Check that pd != 0
        if any(cm[:, 0] != 0):
            print("[Warn] Contains prediction of label 0:", cm[:, 0])
        # Ignore gt == 0
        valid = cm[1:, 1:]
        ious = []
        for c in range(len(valid)):
            intersection = valid[c, c]
            union = np.sum(valid[c, :]) + np.sum(valid[:, c]) - intersection
            if union == 0:
                union = 1
            ious.append(float(intersection) / union)
        return ious

    def get_mean_iou(self):
        per_class_ious = self.get_per_class_ious()
        return np.sum(per_class_ious) / len(per_class_ious)

    def get_accuracy(self):
        """overall accuracy over the points whose label is not 0"""
        valid = self.confusion_matrix[1:, 1:]
        return np.trace(valid) / np.sum(valid)

    def print_metrics(self, labels=None):
        cm = self.confusion_matrix
        # 1. Confusion matrix
        print("Confusion matrix:")
        # Fill default labels: ["0", "1", "2", ...]
        if labels is None:
            labels = [str(val) for val in range(self.num_classes)]
        elif len(labels) != self.num_classes:
            raise ValueError("len(labels) != self.num_classes")
        column_width = max([len(x) for x in labels] + [7])
        empty_cell = " " * column_width
        print("    " + empty_cell, end=" ")
        for label in labels:
            print("%{0}s".format(column_width) % label, end=" ")
        print()
        for i, label in enumerate(labels):
            print("    %{0}s".format(column_width) % label, end=" ")
            for j in range(len(labels)):
                cell = "%{0}.0f".format(column_width) % cm[i, j]
                print(cell, end=" ")
            print()
        # 2. IoU per class
        print("IoU per class:")
        pprint(self.get_per_class_ious())
        # 3. Mean IoU (excluding class 0)
        print("mIoU (ignoring label 0):")
        print(self.get_mean_iou())
        # 4. Overall accuracy
        print("Overall accuracy")
        print(self.get_accuracy())


def epoch_log_lines(mean_loss, per_class_iou, accuracy, mean_iou, labels_names=SEMANTIC3D_LABELS_NAMES):
    """the lines the reference's train_one_epoch / eval_one_epoch log (train.py:250-256, 318-327); per_class_iou: classes
    1 .. C-1 (get_per_class_ious)"""
    lines = ["mean loss: %f" % mean_loss, "Overall accuracy : %f" % accuracy, "Average IoU : %f" % mean_iou]
    iou = [0] + list(per_class_iou)  # label 0 is ignored
    for i in range(1, len(iou)):
        lines.append("IoU of %s : %f" % (labels_names[i], iou[i]))
    return lines
