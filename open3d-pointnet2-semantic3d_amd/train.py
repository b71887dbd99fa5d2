"""One data-parallel training step of the SSG network (BASELINE config[3]).

Restates what train.py of the reference does per batch (train.py:80-119 schedules, :381-388 Adam +
minimize, model.py:152-161 loss) on the MI355X layer API: forward with batch-statistic BatchNorm
(HIP index/gather kernels + differentiable torch layers), weighted sparse softmax cross-entropy,
backward through the HIP gradient kernels (group_point_grad, gather_point_grad,
three_interpolate_grad, pn2_linear_dgrad / _wgrad), a two-bucket RCCL all-reduce overlapped with backward, Adam or momentum.
"""
from collections import OrderedDict

import torch

from . import dist as pdist
from . import model
from ._lib import launch, ptr
from .util import metric, tf_util


def learning_rate(step, batch_size, base_lr=1e-3, decay_step=200000, decay_rate=0.7, floor=1e-5):
    """tf.train.exponential_decay(staircase=True) clipped at 1e-5 (train.py:80-98)."""
    return max(base_lr * decay_rate ** ((step * batch_size) // decay_step), floor)


def bn_decay(step, batch_size, init=0.5, decay_step=200000, decay_rate=0.5, clip=0.99):
    """bn_decay = min(clip, 1 - init * rate^floor(step*B/decay_step)) (train.py:101-119)."""
    return min(clip, 1.0 - init * decay_rate ** ((step * batch_size) // decay_step))


def adam_lr_t(lr, t, beta1=0.9, beta2=0.999):
    """tf.train.AdamOptimizer's per-step rate: lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = 1, 2, ..."""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


class Trainer:
    """One process per GPU.  Everything between the input batch and the updated weights runs on the HIP library:
    forward GEMMs (pn2_linear), batch-norm kernels, weighted CE (pn2_weighted_ce_*), dropout (pn2_dropout), data and
    weight gradients (pn2_linear_dgrad / _wgrad), index-op gradients, and ONE optimizer launch over flat parameter / slot
    buffers.  torch supplies memory, streams, the autograd tape and torch.distributed.

    The optimizer is the reference's choice (semantic.json "optimizer", train.py:380-388): "adam" (the default) is
    tf.train.AdamOptimizer -- pn2_adam_step over flat_p and the slots flat_m, flat_v, device scalars [lr_t, beta1, beta2, eps,
    1/world]; "momentum" is tf.train.MomentumOptimizer(lr, momentum=hp["momentum"]) -- pn2_momentum_step over flat_p and the
    one slot flat_accum, device scalars [lr, momentum, 1/world], the plain scheduled rate with no bias correction.  `slots`
    maps the slot names ("m", "v" / "accum") to their flat buffers.

    Step-dependent scalars live in device memory (the optimizer's learning rate, dropout step), so after
    `warmup_eager` ordinary steps the step is captured and replayed: on one GPU as ONE hipGraph; with several ranks as three
    (forward + head/FP backward | SA backward | Adam) with the two buckets' all-reduces between them, the first one
    asynchronous so that it travels while the second graph replays -- no collective inside a captured region.  Eager steps
    (the warm-up, capture=False) launch the first bucket's all-reduce from inside backward (dist.OverlappedGradAllReduce).

    Metrics (the reference's train_one_epoch / eval_one_epoch, train.py:199-331): with track_metrics=True every training step
    also counts the argmax of its logits against the labels into `train_confusion` (util.metric.ConfusionMatrix on the device)
    and adds its loss to a device [sum, count] -- one pn2_confusion_update launch right after the loss, inside whichever graphs
    the step is captured into; `train_metrics()` reads them (the one synchronisation), `reset_metrics()` starts an epoch.
    `eval_step` is the validation forward (inference mode) + loss + the same counting into `eval_confusion`.

    Stopping and continuing (what the reference's tf.train.Saver checkpoint holds): `state_dict()` / `save(path)` give the
    variables, the moving averages, the optimizer slots by variable name and the step count -- which drives the learning-rate
    staircase, the batch-norm decay, Adam's bias correction and the dropout stream; `load_state_dict(state)` / `load(path)` put
    them into a fresh trainer (applied when its first batch creates the variables) or, in place, into a live one."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-8  # tf.train.AdamOptimizer defaults (train.py:381-384)

    def __init__(self, hyperparams, num_class, store=None, device="cuda", capture=True, warmup_eager=3,
                 split_capture=None, overlap_collective=True, track_metrics=False):
        self.hp = dict(hyperparams)
        # schedule / optimizer keys of the reference's semantic.json (train.py:80-119, 380-386); its defaults when absent
        opt = str(self.hp.get("optimizer", "adam")).lower()
        if opt not in ("adam", "momentum"):
            raise ValueError("optimizer %r: 'adam' (the reference's semantic.json setting, train.py:385-386) and 'momentum' "
                             "(train.py:380-383) are built" % (opt,))
        self.optimizer = opt
        self.momentum = float(self.hp.get("momentum", 0.9))
        self.sched = dict(base_lr=float(self.hp.get("learning_rate", 1e-3)), decay_step=int(self.hp.get("decay_step", 200000)),
                          lr_decay_rate=float(self.hp.get("learning_rate_decay_rate", 0.7)),
                          bn_init=float(self.hp.get("bn_init_decay", 0.5)), bn_rate=float(self.hp.get("bn_decay_decay_rate", 0.5)),
                          bn_clip=float(self.hp.get("bn_decay_clip", 0.99)))
        self.num_class = num_class
        self.store = store or tf_util.set_default_store(tf_util.VariableStore(device=device, seed=0))
        self.step_count = 0
        self._steps_run = 0  # steps THIS object has run (= step_count unless a state was loaded): what warmup_eager counts, so
                             # that a resumed trainer also warms up eagerly before it captures
        self.bucket = None
        self.flat_p, self.flat_m, self.flat_v, self.flat_accum, self.slots = None, None, None, None, None
        self._var_slices, self._pending_state = None, None
        self.capture, self.warmup_eager = bool(capture), int(warmup_eager)
        self._graph, self._graph_decay, self._static, self._stream = None, None, None, None
        self._static_geo, self._geo, self._geo_tag, self._geo_event, self._geo_stream = None, None, None, None, None
        # split_capture: the step as TWO graphs -- forward + backward (gradients packed, no collective inside), then Adam --
        # with the gradient all-reduce launched between them: how a step is captured when there are several ranks (a
        # collective inside a captured backward pass is avoided).  None = when world > 1; True forces it (tests).
        self.split_capture = split_capture
        # overlap_collective (with a split capture): THREE graphs -- forward + the backward pass down to the FP / SA boundary |
        # the SA part of the backward pass | Adam -- so that the all-reduce of the head + FP gradients (launched asynchronously
        # after the first) travels while the second replays; the SA bucket's all-reduce follows it.  False: two graphs around
        # ONE all-reduce of the whole flat gradient.
        self.overlap_collective = bool(overlap_collective)
        self._graph_adam, self._graph_late = None, None
        # staging (single-graph capture): the NEXT batch -- inputs, geometry, Adam's lr_t, the dropout step -- is put into staging
        # buffers by the geometry stream while this step runs; a one-node copy graph moves it into the step's static buffers.  The
        # trainer's stream then carries graphs only: an eager launch between two replays costs ~0.1 ms of idle queue (measured:
        # the captured step replays back to back in 3.33 ms, with one eager copy in between 3.45), a graph after a graph nothing.
        self._copy_graph, self._staging, self._staged_tag, self._copied_event = None, None, None, None
        # comm_events (bench.py --train): a list that receives, per captured multi-rank step, three HIP events on the
        # trainer's stream: early bucket launched | SA backward graph done | both buckets reduced
        self.comm_events = None
        self._world0 = None
        # metrics: off by default (the step and its graphs are then exactly what they are without this code)
        self.track_metrics = bool(track_metrics)
        self.train_confusion, self._train_loss_acc, self.last_logits = None, None, None
        self.eval_confusion, self._eval_loss_acc, self.last_eval_logits = None, None, None
        self._eval_graph, self._eval_static, self._eval_key, self._eval_warm_key = None, None, None, None

    # ---- set-up ------------------------------------------------------------------------------------------------
    def _lazy_init(self, pc):
        # variables are created by the first forward (TF-style get_variable semantics).  That forward must leave no
        # trace: no autograd graph, and the moving averages restored (the reference applies ONE update per step,
        # train.py:381-388; the HIP BN kernel updates them through raw pointers even under no_grad).
        tf_util.set_default_store(self.store)
        with torch.no_grad():
            before = {k: v.clone() for k, v in self.store.buffers.items()}  # a pre-loaded store keeps its statistics
            model.get_model(pc[:1], True, self.num_class, self.hp, bn_decay=self._bn_decay(0, pc.shape[0]))
            for k, v in self.store.buffers.items():
                if k in before:
                    v.copy_(before[k])
                else:
                    v.fill_(0.0 if k.endswith("moving_mean") else 1.0)  # tf_util.py:571-581 initial moving averages
        names = list(self.store.params.keys())
        params = self.store.parameters()
        pdist.broadcast_parameters(params)
        pdist.broadcast_parameters(list(self.store.buffers.values()))
        # flat parameter / moment buffers: every parameter becomes a view of `flat_p` (same Parameter objects)
        dev = params[0].device
        n = sum(p.numel() for p in params)
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        off = 0
        self._var_slices = OrderedDict()  # variable name -> (offset, numel, shape) in flat_p and in every slot buffer
        with torch.no_grad():
            for name, p in zip(names, params):
                v = self.flat_p[off:off + p.numel()].view_as(p)
                v.copy_(p)
                p.data = v
                self._var_slices[name] = (off, p.numel(), tuple(p.shape))
                off += p.numel()
        # the optimizer's slots, flat like the parameters: Adam's two moments, or momentum's one accumulator
        if self.optimizer == "adam":
            self.flat_m = torch.zeros_like(self.flat_p)
            self.flat_v = torch.zeros_like(self.flat_p)
            self.slots = OrderedDict([("m", self.flat_m), ("v", self.flat_v)])
        else:
            self.flat_accum = torch.zeros_like(self.flat_p)
            self.slots = OrderedDict([("accum", self.flat_accum)])
        # backward reaches the head and the FP layers first: they are the early bucket (created after layer1..layer4)
        split = next((i for i, k in enumerate(names) if not k.startswith("layer")), len(names))
        self.bucket = pdist.OverlappedGradAllReduce(params, split)
        # the gradient kernels write every parameter's gradient straight into its slice of the bucket's flat buffer
        # (tf_util.VariableStore.grad_view): backward leaves nothing to pack
        off = 0
        for p in self.bucket.params:
            self.store.grad_map[p.data_ptr()] = (self.bucket.flat, off, p.numel())
            off += p.numel()
        # pn2_adam_step's device-side scalars: [lr_t, beta1, beta2, eps, grad_scale].  Only lr_t changes per step; it is
        # written with a fill whose value travels BY VALUE in the launch (no host buffer a run-ahead host could rewrite
        # before an asynchronous copy has read it: with sync=False the host is several steps ahead of the device).
        # pn2_momentum_step's: [lr, momentum, grad_scale], the per-step slot first as well.
        scalars = [self.BETA1, self.BETA2, self.EPS] if self.optimizer == "adam" else [self.momentum]
        self.hyper = torch.tensor([0.0] + scalars + [1.0 / self.bucket.world()], dtype=torch.float32).to(dev)
        self._lr_slot = self.hyper[0:1]
        self._world0 = self.bucket.world()  # frozen into grad_scale above: a process group created later would mis-scale
        self._stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        self._geo_stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        if self.track_metrics:
            # fixed device buffers: a captured step adds into these addresses on every replay (reset zeroes them in place)
            self.train_confusion = metric.ConfusionMatrix(self.num_class, device=dev)
            self._train_loss_acc = torch.zeros(2, dtype=torch.float64, device=dev)
        if self._pending_state is not None:
            # a state loaded before the variables existed: in place of the initial moments and moving averages
            state, self._pending_state = self._pending_state, None
            self._check_state(state)
            self._apply_state(state)

    def _learning_rate(self, step, batch_size):
        c = self.sched
        return learning_rate(step, batch_size, c["base_lr"], c["decay_step"], c["lr_decay_rate"])

    def _bn_decay(self, step, batch_size):
        c = self.sched
        return bn_decay(step, batch_size, c["bn_init"], c["decay_step"], c["bn_rate"], c["bn_clip"])

    def _optimizer_lr(self, step, batch_size):
        """what the lr slot (hyper[0]) holds for 0-based step `step`: Adam's bias-corrected rate of time step `step` + 1, or, for
        momentum, the plain scheduled rate"""
        lr = self._learning_rate(step, batch_size)
        return adam_lr_t(lr, step + 1, self.BETA1, self.BETA2) if self.optimizer == "adam" else lr

    # ---- one step ------------------------------------------------------------------------------------------------
    def _forward_backward(self, pc, labels, smpw, decay, geometry=None):
        if self.store.zero_arena is None:
            self.store.zero_arena = tf_util.ZeroArena(self.flat_p.device)  # first step: measures what the step needs
        elif self.store.zero_arena.buf is None:
            self.store.zero_arena.allocate()
        self.store.zero_arena.reset()  # ONE zero fill for every accumulator of the step
        self.bucket.flat.zero_()       # and one for the flat gradient the weight-gradient kernels add into
        for p in self.bucket.params:
            p.grad = None
        self.store.grad_direct = True
        try:
            logits, _ = model.get_model(pc, True, self.num_class, self.hp, bn_decay=decay, geometry=geometry)
            loss = model.get_loss(logits, labels, smpw)
            if self.track_metrics:
                self._count_train(logits, labels, loss)
            self.bucket.begin()
            loss.backward()
        finally:
            self.store.grad_direct = False
        return loss.detach(), self.bucket.finish()

    def _forward_backward_early(self, pc, labels, smpw, decay, geometry=None):
        """first piece of a cut step: forward, loss, and the backward pass of the head and the FP modules down to (detached
        copies of) the SA outputs; the early bucket is packed.  -> loss"""
        if self.store.zero_arena is None:
            self.store.zero_arena = tf_util.ZeroArena(self.flat_p.device)
        elif self.store.zero_arena.buf is None:
            self.store.zero_arena.allocate()
        self.store.zero_arena.reset()
        self.bucket.flat.zero_()
        for p in self.bucket.params:
            p.grad = None
        self.store.grad_direct = True
        try:
            logits, ep = model.get_model(pc, True, self.num_class, self.hp, bn_decay=decay, geometry=geometry, cut_sa_fp=True)
            loss = model.get_loss(logits, labels, smpw)
            if self.track_metrics:
                self._count_train(logits, labels, loss)
            early = list(self.bucket.params[self.bucket.split:])
            cut = list(ep["sa_features_cut"])
            grads = torch.autograd.grad(loss, early + cut, allow_unused=True)
        finally:
            self.store.grad_direct = False
        for p, g in zip(early, grads[:len(early)]):
            p.grad = g
        self.bucket.pack_early()
        self._cut = [(t, g) for t, g in zip(ep["sa_features"][1:], grads[len(early):]) if g is not None]
        return loss.detach()

    def _count_train(self, logits, labels, loss):
        """the step's metrics: argmax of the training-mode logits vs the labels into train_confusion, loss into [sum, count].
        last_logits keeps the logits alive (and, while capturing, keeps the graph pool from reusing their memory)."""
        self.last_logits = logits.detach()
        metric.confusion_update(self.last_logits, labels, confusion=self.train_confusion.matrix_tensor,
                                invalid=self.train_confusion.invalid_tensor, loss=loss.detach(), loss_acc=self._train_loss_acc)

    def _backward_late(self):
        """second piece: the SA modules' backward pass from the gradients at the cut; the late bucket is packed"""
        self.store.grad_direct = True
        try:
            torch.autograd.backward([t for t, _ in self._cut], [g for _, g in self._cut])
        finally:
            self.store.grad_direct = False
        self._cut = None
        return self.bucket.pack_late_and_bind()

    def _adam(self, flat_g):
        """the optimizer's apply step (the name is the Adam-only trainer's): ONE launch of the selected entry point"""
        if self.optimizer == "adam":
            launch("pn2_adam_step", self.flat_p, self.flat_p.numel(), ptr(self.flat_p), ptr(flat_g), ptr(self.flat_m), ptr(self.flat_v),
                   ptr(self.hyper))
        else:
            launch("pn2_momentum_step", self.flat_p, self.flat_p.numel(), ptr(self.flat_p), ptr(flat_g), ptr(self.flat_accum),
                   ptr(self.hyper))

    def _step_body(self, pc, labels, smpw, decay, geometry=None):
        loss, flat_g = self._forward_backward(pc, labels, smpw, decay, geometry)
        self._adam(flat_g)
        return loss

    # ---- geometry prefetch -----------------------------------------------------------------------------------------
    def _xyz_of(self, pc):
        return pc[:, :, 0:3].contiguous() if self.hp["use_color"] else pc.contiguous()

    @staticmethod
    def _tag(pc):
        return (pc.data_ptr(), pc._version, tuple(pc.shape))

    def _geometry_for(self, pc, caller):
        """geometry of THIS batch: taken from the prefetch when `pc` is the tensor announced as `next_pc` by the previous
        call, computed now otherwise.  Returns with `caller` (a stream) ordered after its completion."""
        tag = (pc.data_ptr(), pc._version, tuple(pc.shape))
        if self._geo is not None and self._geo_tag == tag:
            caller.wait_event(self._geo_event)
            geo = self._geo
            for t in model.geometry_tensors(geo):
                t.record_stream(caller)  # allocated on the side stream, consumed on this one
        else:
            geo = model.compute_geometry(self._xyz_of(pc), self.hp, plans=True)
        self._geo, self._geo_tag = None, None
        return geo

    def _prefetch(self, next_pc, after_event, next_labels=None, next_smpw=None):
        """launch the geometry of the NEXT batch on the side stream; it may start once `after_event` has passed (the
        consumer of the previous prefetch has taken its copy).  With the whole next batch announced (labels, weights) and a
        captured step with staging buffers, the batch, its geometry and the next step's scalars are also put into the staging
        buffers there: the next call then launches graphs only."""
        self._staged_tag = None
        if next_pc is None:
            return
        g = self._geo_stream
        g.wait_event(after_event)
        with torch.cuda.stream(g):
            self._geo = model.compute_geometry(self._xyz_of(next_pc), self.hp, plans=True)
            stg = self._staging
            if (stg is not None and next_labels is not None and next_smpw is not None and self._copied_event is not None
                    and all(a.shape == d.shape and a.dtype == d.dtype and a.is_contiguous()
                            for a, d in zip((next_pc, next_labels, next_smpw), stg["inputs"]))):
                g.wait_event(self._copied_event)  # the copy graph that read the staging buffers last has run
                srcs = [next_pc, next_labels, next_smpw] + model.geometry_tensors(self._geo)
                dsts = stg["inputs"] + stg["geo"]
                if len(srcs) == len(dsts):
                    nxt = self.step_count + 1  # the step this batch is for (0-based), its Adam time step is nxt + 1
                    lr_t = self._optimizer_lr(nxt, next_pc.shape[0])
                    fills = [(stg["lr"], lr_t)] + [(t, nxt) for t in stg["steps"]]
                    tf_util.multi_copy_(dsts, srcs, fills=fills)
                    self._staged_tag = (self._tag(next_pc), self._tag(next_labels), self._tag(next_smpw), nxt)
            self._geo_event = torch.cuda.Event()
            self._geo_event.record(g)
        self._geo_tag = (next_pc.data_ptr(), next_pc._version, tuple(next_pc.shape))

    def prefetch_geometry(self, next_pc):
        """Announce the next batch AFTER the current step was enqueued (e.g. when it is itself produced on another stream,
        examples/train_synthetic.py): its geometry chain starts once the work queued so far on the CURRENT stream is done."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._prefetch(next_pc, ev)

    def train_step(self, pc, labels, smpw, sync=True, next_pc=None, next_labels=None, next_smpw=None):
        """pc (B,N,6) float32, labels (B,N) int, smpw (B,N) float32 -> loss (python float; the device scalar when
        sync=False, to be read after the next synchronisation point).
        next_pc: the point cloud of the NEXT call (optional).  Its FPS / ball-query / three_nn chain -- weight-independent,
        latency-bound, 16 of 256 CUs -- then runs on a side stream beside this step's dense work instead of in front of
        the next one (what the reference's mp.Pool data loader does for its CPU pre-processing).  next_labels / next_smpw
        (optional, with next_pc): the rest of the next batch; a captured step then finds the whole batch staged and launches
        graphs only (see _prefetch)."""
        tf_util.set_default_store(self.store)
        if self.bucket is None:
            self._lazy_init(pc)
        b = pc.shape[0]
        world = self.bucket.world()
        if world != self._world0 and not self.bucket.skip_collectives:
            raise RuntimeError("the process group changed after the trainer's first step (world %d -> %d): the gradient scale "
                               "1/world is part of the optimizer state; build a new Trainer" % (self._world0, world))
        decay = self._bn_decay(self.step_count, b)
        lr_t = self._optimizer_lr(self.step_count, b)  # the eager fill and the fills= between graphs below write this value
        use_graph = self.capture and pc.is_cuda and self._steps_run >= self.warmup_eager
        split = use_graph and (world > 1 if self.split_capture is None else bool(self.split_capture))
        caller = torch.cuda.current_stream()
        if not use_graph:
            self._lr_slot.fill_(lr_t)
            self.store.set_step(self.step_count)
            geo = self._geometry_for(pc, caller)
            taken = torch.cuda.Event()
            taken.record(caller)
            self._prefetch(next_pc, taken)  # (an eager step has no staging buffers)
            loss = self._step_body(pc, labels, smpw, decay, geometry=geo)
        else:
            # Replays and the per-step writes they depend on run on the trainer's OWN stream.  Launching the graph into
            # the null stream is not safe on this stack: work queued on the null stream after hipGraphLaunch started
            # before the graph had finished (the next step's input copy then faulted with "write access to a read-only
            # page" around the 13th replay; a device-wide synchronise in between hid it).
            self._stream.wait_stream(caller)
            with torch.cuda.stream(self._stream):
                recapture = self._graph is None or self._graph_decay != decay or self._static[0].shape != pc.shape
                staged = (not recapture and self._copy_graph is not None and self._staged_tag is not None and self._staged_tag ==
                          (self._tag(pc), self._tag(labels), self._tag(smpw), self.step_count))
                if staged:
                    # the geometry stream has put this batch, its geometry and this step's scalars into the staging buffers:
                    # copy graph -> step graph, no eager launch on this stream
                    self._stream.wait_event(self._geo_event)
                    self._geo, self._geo_tag, self._staged_tag = None, None, None
                    self._copy_graph.replay()
                    self._copied_event = torch.cuda.Event()
                    self._copied_event.record(self._stream)
                    self._prefetch(next_pc, self._copied_event, next_labels, next_smpw)
                    self._graph.replay()
                    loss = self._static[3]
                    if sync:
                        loss = float(loss)
                    caller.wait_stream(self._stream)
                    self.step_count += 1
                    self._steps_run += 1
                    self.store.train_epoch += 1
                    return float(loss) if sync else loss
                geo = self._geometry_for(pc, self._stream)  # eager (or eagerly prefetched: prefetch_geometry)
                if recapture:
                    self._capture(pc, labels, smpw, decay, geo, split)
                # every per-step device-to-device copy (inputs, and this batch's geometry when it is not in place yet) AND the
                # step's scalars (Adam's lr_t, the dropout step: their values travel in the launch arguments) in ONE launch: they
                # sit between two graphs on the critical path
                pairs = [(d, s_) for d, s_ in zip(self._static[:3], (pc, labels, smpw))
                         if d.data_ptr() != s_.data_ptr() and s_.is_contiguous() and s_.dtype == d.dtype]
                for d, s_ in zip(self._static[:3], (pc, labels, smpw)):
                    if d.data_ptr() != s_.data_ptr() and not (s_.is_contiguous() and s_.dtype == d.dtype):
                        d.copy_(s_, non_blocking=True)
                pairs += list(zip(model.geometry_tensors(self._static_geo), model.geometry_tensors(geo)))
                fills = [(self._lr_slot, lr_t)] + self.store.step_fills(self.step_count)
                if pairs and len(fills) <= 4:
                    tf_util.multi_copy_([d for d, _ in pairs], [s_ for _, s_ in pairs], fills=fills)
                else:
                    self._lr_slot.fill_(lr_t)
                    self.store.set_step(self.step_count)
                    if pairs:
                        tf_util.multi_copy_([d for d, _ in pairs], [s_ for _, s_ in pairs])
                taken = torch.cuda.Event()
                taken.record(self._stream)
                self._copied_event = taken  # (nothing reads the staging buffers in this form of the step)
                self._prefetch(next_pc, taken, next_labels, next_smpw)
                self._graph.replay()
                if self._graph_late is not None:  # three segments: the early bucket travels while the SA backward replays
                    ev = self.comm_events  # bench: [(early launched, SA backward done, both buckets reduced)] per step
                    if ev is not None:
                        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                        e0.record(self._stream)
                    work = self.bucket.reduce_early_async()
                    self._graph_late.replay()
                    if ev is not None:
                        e1.record(self._stream)
                    self.bucket.reduce_late_and_wait(work)
                    if ev is not None:
                        e2.record(self._stream)
                        ev.append((e0, e1, e2))
                    self._graph_adam.replay()
                elif self._graph_adam is not None:  # split capture: the collective runs between the two graphs
                    self.bucket.reduce_deferred()
                    self._graph_adam.replay()
                loss = self._static[3]
                if sync:
                    loss = float(loss)
            caller.wait_stream(self._stream)
        self.step_count += 1
        self._steps_run += 1
        # A replayed graph updates parameters and moving averages through raw pointers: neither a tensor version counter
        # nor the training-mode layer calls (which only run while capturing) tell the inference-weight cache
        # (VariableStore.folded) that they changed.  Every step does.
        self.store.train_epoch += 1
        return float(loss) if sync else loss

    def _capture(self, pc, labels, smpw, decay, geo, split=False):
        """record forward + loss + backward + Adam of one step into a hipGraph (static input and geometry buffers); split:
        Adam in a graph of its own, the gradient all-reduce is launched between the two replays."""
        torch.cuda.synchronize()
        st = [pc.clone(), labels.clone(), smpw.clone()]
        sg = model.clone_geometry(geo, self._xyz_of(st[0]))
        for p in self.bucket.params:
            p.grad = None
        # capture_error_mode thread_local: with a process group alive, RCCL's watchdog thread polls the events of earlier
        # collectives (hipEventQuery); under the default GLOBAL mode that call is illegal while ANY thread captures and takes the
        # process down (seen as an abort in destroy_process_group after a full test session)
        mode = dict(capture_error_mode="thread_local")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **mode):
            if split and self.overlap_collective:
                loss = self._forward_backward_early(st[0], st[1], st[2], decay, geometry=sg)
            elif split:
                self.bucket.defer_collectives = True
                try:
                    loss, flat_g = self._forward_backward(st[0], st[1], st[2], decay, geometry=sg)
                finally:
                    self.bucket.defer_collectives = False
            else:
                loss = self._step_body(st[0], st[1], st[2], decay, geometry=sg)
        self._graph_adam, self._graph_late = None, None
        if split and self.overlap_collective:
            gl = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gl, pool=g.pool(), **mode):
                flat_g = self._backward_late()
            self._graph_late = gl
        if split:
            ga = torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga, **mode):
                self._adam(flat_g)
            self._graph_adam = ga
        self._graph, self._graph_decay, self._static, self._static_geo = g, decay, st + [loss], sg
        # staging buffers + the one-node copy graph (single-graph capture only: a multi-rank step has collectives between its
        # graphs anyway)
        self._copy_graph, self._staging, self._staged_tag = None, None, None
        if not split:
            steps = [t[1:2] for t in self.store._dropout.values()]
            dsts = st + model.geometry_tensors(sg) + [self._lr_slot] + steps
            stg = {"inputs": [t.clone() for t in st], "geo": [t.clone() for t in model.geometry_tensors(sg)],
                   "lr": self._lr_slot.clone(), "steps": [t.clone() for t in steps]}
            srcs = stg["inputs"] + stg["geo"] + [stg["lr"]] + stg["steps"]
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc, **mode):
                tf_util.multi_copy_(dsts, srcs)
            self._copy_graph, self._staging = gc, stg
        # the capture itself executed nothing: the replay that follows is this step

    # ---- stop and continue -----------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Everything a stopped run continues from (the content of the reference's tf.train.Saver checkpoint), as CPU tensors and
        Python scalars:
          "variables":     store.state_dict() -- parameters and moving averages by variable name;
          "optimizer":     {"name": "adam" | "momentum", "slots": {"<var>/m", "<var>/v" | "<var>/accum": tensor}} -- TF's
                           <var>/Adam, <var>/Adam_1 | <var>/Momentum; by variable, so a file does not depend on the flat layout;
          "step_count":    the number of steps taken;
          "dropout_seeds": {site: seed word} of every dropout site, so that a store with another seed refuses the state instead
                           of drawing other masks.
        The world size (grad_scale) is not part of it.  One synchronisation."""
        if self.bucket is None:
            raise RuntimeError("this trainer has no variables yet: they are created by its first batch (train_step / eval_step)")

        def read():
            variables = {k: v.cpu() for k, v in self.store.state_dict().items()}
            slots = {}
            for var, (off, n, shape) in self._var_slices.items():
                for slot, flat in self.slots.items():
                    slots["%s/%s" % (var, slot)] = flat[off:off + n].view(shape).cpu()
            seeds = {str(k): int(t[0]) for k, t in self.store._dropout.items()}
            return {"variables": variables, "optimizer": {"name": self.optimizer, "slots": slots},
                    "step_count": int(self.step_count), "dropout_seeds": seeds}
        return self._on_trainer_stream(read)

    def _check_state(self, state):
        """ValueError unless `state` fits this trainer: same optimizer, same variables and slots with the same shapes, same
        dropout seeds.  Called before anything is written."""
        name = state["optimizer"]["name"]
        if name != self.optimizer:
            raise ValueError("the state was saved by optimizer %r, this trainer runs %r" % (name, self.optimizer))
        have = OrderedDict((k, tuple(v.shape)) for k, v in list(self.store.params.items()) + list(self.store.buffers.items()))
        for what, want, got in (("variables", have, state["variables"]),
                                ("optimizer slots", {"%s/%s" % (var, slot): shape for var, (_, _, shape) in self._var_slices.items()
                                                     for slot in self.slots}, state["optimizer"]["slots"])):
            if set(want) != set(got):
                diff = sorted(set(want) ^ set(got))
                raise ValueError("the state's %s differ from this trainer's: %s%s" % (what, ", ".join(diff[:4]),
                                                                                     " ..." if len(diff) > 4 else ""))
            for k, shape in want.items():
                if tuple(got[k].shape) != shape:
                    raise ValueError("%s: the state holds shape %s, this trainer %s" % (k, tuple(got[k].shape), shape))
        seeds = {str(k): int(t[0]) for k, t in self.store._dropout.items()}
        if {str(k): int(v) for k, v in state["dropout_seeds"].items()} != seeds:
            raise ValueError("the state's dropout seeds differ from this store's (a VariableStore built with another seed): "
                             "the continued run would draw other masks")

    def _apply_state(self, state):
        """copy a checked state into the EXISTING buffers (captured graphs hold their addresses) and set the step count"""
        dev = self.flat_p.device

        def write():
            with torch.no_grad():
                for k, v in state["variables"].items():
                    self.store.params.get(k, self.store.buffers.get(k)).copy_(v.to(dev))
                for var, (off, n, shape) in self._var_slices.items():
                    for slot, flat in self.slots.items():
                        flat[off:off + n].view(shape).copy_(state["optimizer"]["slots"]["%s/%s" % (var, slot)].to(dev))
        self._on_trainer_stream(write)
        self.step_count = int(state["step_count"])
        self.store.train_epoch += 1  # parameters and moving averages changed under the folded inference weights
        # a prefetched or staged next batch carries the learning rate and dropout step of the old step count
        self._geo, self._geo_tag, self._staged_tag = None, None, None

    def load_state_dict(self, state):
        """Continue from `state` (a state_dict()).  On a trainer that has stepped, everything is copied in place -- no buffer moves,
        the captured graphs stay valid; the next train_step recaptures by itself only if the batch-norm decay of the new step
        differs.  On a fresh trainer the state is kept and applied when the first batch has created the variables, in place of
        their initial moments and moving averages (that call then raises what this one would have).  ValueError, with nothing
        loaded: another optimizer, other variable names or shapes, other dropout seeds.  The world size may differ."""
        name = state["optimizer"]["name"]
        if name != self.optimizer:
            raise ValueError("the state was saved by optimizer %r, this trainer runs %r" % (name, self.optimizer))
        if self.bucket is None:
            self._pending_state = state
            return
        self._check_state(state)
        self._apply_state(state)

    def save(self, path):
        """torch.save of state_dict(): tensors, strings, ints and floats only"""
        torch.save(self.state_dict(), path)

    def load(self, path):
        """load_state_dict of a file written by save()"""
        self.load_state_dict(torch.load(path, weights_only=True, map_location="cpu"))

    # ---- metrics and validation ----------------------------------------------------------------------------------------------
    def _on_trainer_stream(self, fn):
        """run fn() on the trainer's stream, ordered after the caller's work so far and before the caller's later work (the
        replays of train_step / eval_step run on that stream too)"""
        caller = torch.cuda.current_stream()
        st = self._stream if self._stream is not None else caller
        st.wait_stream(caller)
        with torch.cuda.stream(st):
            out = fn()
        caller.wait_stream(st)
        return out

    def reset_metrics(self):
        """start a training epoch: zero train_confusion and the loss sums, behind every step enqueued so far and in front of
        every later one (a fill on the trainer's stream; no synchronisation)"""
        if self.train_confusion is None:
            raise RuntimeError("this trainer was built with track_metrics=False")
        self._on_trainer_stream(lambda: (self.train_confusion.reset(), self._train_loss_acc.zero_()))

    def reset_eval_metrics(self):
        """start a validation pass: zero eval_confusion and its loss sums (ordered as reset_metrics)"""
        if self.eval_confusion is not None:
            self._on_trainer_stream(lambda: (self.eval_confusion.reset(), self._eval_loss_acc.zero_()))

    def train_metrics(self):
        """{mean_loss, accuracy, mean_iou, per_class_iou} of the training steps since the last reset_metrics (plus
        confusion_matrix, num_invalid, steps), summed over the ranks when there are several.  The one synchronisation."""
        if self.train_confusion is None:
            raise RuntimeError("this trainer was built with track_metrics=False")
        return self._read_metrics(self.train_confusion, self._train_loss_acc)

    def eval_metrics(self):
        """the same for the eval_step calls since the last reset_eval_metrics"""
        if self.eval_confusion is None:
            raise RuntimeError("no eval_step has run")
        return self._read_metrics(self.eval_confusion, self._eval_loss_acc)

    def _read_metrics(self, cm, acc):
        import numpy as np
        c = self.num_class
        caller = torch.cuda.current_stream()
        if self._stream is not None:
            caller.wait_stream(self._stream)
        # counts and loss sums in ONE float64 buffer (counts below 2^53 are exact): one all-reduce, one read-back
        packed = torch.cat([cm.counts[:c * c + 1].double(), acc])
        if self.bucket is not None and self.bucket.world() > 1:
            import torch.distributed as tdist
            tdist.all_reduce(packed)
        host = packed.cpu().numpy()
        out_cm = metric.ConfusionMatrix(c)
        out_cm.confusion_matrix = np.rint(host[:c * c]).astype(np.int64).reshape(c, c)
        ious = out_cm.get_per_class_ious()
        with np.errstate(invalid="ignore", divide="ignore"):
            accuracy = float(out_cm.get_accuracy())
        steps = int(round(host[c * c + 2]))
        return {"mean_loss": float(host[c * c + 1] / steps) if steps else float("nan"), "accuracy": accuracy,
                "mean_iou": float(np.sum(ious) / len(ious)) if ious else float("nan"), "per_class_iou": ious,
                "confusion_matrix": out_cm.confusion_matrix, "num_invalid": int(round(host[c * c])), "steps": steps}

    def _eval_body(self, pc, labels, smpw):
        with torch.no_grad():
            logits, _ = model.get_model(pc, False, self.num_class, self.hp)
            loss = model.get_loss(logits, labels, smpw)
            self.last_eval_logits = logits
            metric.confusion_update(logits, labels, confusion=self.eval_confusion.matrix_tensor,
                                    invalid=self.eval_confusion.invalid_tensor, loss=loss, loss_acc=self._eval_loss_acc)
        return loss

    def eval_step(self, pc, labels, smpw, sync=True):
        """The body of the reference's eval_one_epoch (train.py:262-331) for one batch: the inference forward (is_training=False:
        moving averages, no dropout), the weighted cross-entropy, and the argmax / confusion-matrix update into eval_confusion
        and its loss sums (eval_metrics(), reset_eval_metrics()).  Parameters, moving averages and Adam's moments are not
        touched.  -> loss (python float; with sync=False the device scalar, overwritten by the next eval_step).

        The first call for a given set of weights and shapes runs eagerly (it also fills the folded-inference-weight cache); the
        next captures the pass into a graph and later calls replay it.  Any training step changes the weights (VariableStore
        .train_epoch): the graph, which reads the folded weights of its capture, is then dropped and built again.

        The reference's validation split has all-zero label weights (dataset/semantic_dataset.py), so the loss it logs for
        validation is 0 under SUM_BY_NONZERO_WEIGHTS (0 / max(1, 0)); pass the weights you want the loss computed with."""
        tf_util.set_default_store(self.store)
        if self.bucket is None:
            self._lazy_init(pc)
        if self.eval_confusion is None:
            dev = self.flat_p.device
            self.eval_confusion = metric.ConfusionMatrix(self.num_class, device=dev)
            self._eval_loss_acc = torch.zeros(2, dtype=torch.float64, device=dev)

        def run():
            if not (self.capture and pc.is_cuda):
                return self._eval_body(pc, labels, smpw)
            key = (self.store.train_epoch,) + tuple((tuple(t.shape), t.dtype) for t in (pc, labels, smpw))
            if self._eval_key != key:  # weights (folded inference weights) or shapes changed since the capture
                self._eval_graph, self._eval_static, self._eval_key = None, None, None
            if self._eval_graph is None and self._eval_warm_key == key:
                self._capture_eval(pc, labels, smpw)
                self._eval_key = key
            if self._eval_graph is None:
                self._eval_warm_key = key
                return self._eval_body(pc, labels, smpw)
            for d, s_ in zip(self._eval_static[:3], (pc, labels, smpw)):
                if d.data_ptr() != s_.data_ptr():
                    d.copy_(s_, non_blocking=True)
            self._eval_graph.replay()
            return self._eval_static[3]

        loss = self._on_trainer_stream(run)
        return float(loss) if sync else loss

    def _capture_eval(self, pc, labels, smpw):
        torch.cuda.synchronize()
        st = [t.contiguous().clone() for t in (pc, labels, smpw)]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            loss = self._eval_body(*st)
        self._eval_graph, self._eval_static = g, st + [loss]
