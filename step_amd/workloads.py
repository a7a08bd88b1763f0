"""step_amd/workloads.py -- synthetic BASELINE workloads C3 (full two_branch inference) and C4 (one training step) built
from the product modules; used by bench.py --config c3|c4 and tools/c3_bench.py.  Random-init weights of the real
architectures, synthetic clips and the reference's default anchor grid (there are no datasets or checkpoints offline)."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from . import BaseNet, ContextNet, ROINet, TwoBranchNet
from . import rng as srng
from . import dist as sdist, wgrad
from .driver import GraphedInference, inference, inference_flat, postprocess
from .backbone import wgrad_into_grad
from .optim import FlatAdam, FlatSGD
from .selection import DeviceClsSelector, DeviceSelector, cls_select, sample_anchors, train_select
from .driver import _flat_tubes, pad_tubes
from .tube_math import ANCHOR_MODES, anchor_tubes, generate_anchors


def step_cfg(**kw):
    """The attributes of the reference's argparse namespace the modules read (config.py; scripts/train_step.sh)."""
    base = dict(base_net="i3d", kinetics_pretrain=None, freeze_stats=True, freeze_affine=True, fp16=False, T=3, num_classes=60,
                fc_dim=256, dropout=0.0, pool_size=7, no_context=False, max_iter=3, NUM_CHUNKS={1: 1, 2: 1, 3: 3, 4: 3},
                temporal_mode="predict", image_size=(400, 400), pool_mode="align",
                # training sample selection (config.py:64-76 with the values of scripts/train_step.sh:43-48)
                topk=-1, cls_thresh=[0.2, 0.35, 0.5], reg_thresh=[0.2, 0.35, 0.5], max_pos_num=5, neg_ratio=2,
                selection_sampling="softmax", lambda_reg=5.0, lambda_neighbor=1.0)
    base.update(kw)
    return NS(**base)


def build_nets(dev, seed=123, heads=3, cls_only=False, **cfg):
    args = step_cfg(**cfg)                                        # (overrides of the recipe: dropout=0.3 is scripts/train_step.sh:41)
    torch.manual_seed(seed)                                       # config.py:38 man_seed
    base = BaseNet(args).to(dev).eval()
    ctx = ContextNet(args).to(dev).eval()
    nets = {"roi_net": ROINet("align", 7)}
    for i in range(heads):
        d = (TwoBranchNet(args, cls_only=True) if cls_only else TwoBranchNet(args)).to(dev).eval()      # (cls_only: train_cls.py:97)
        d.set_device(dev)
        nets["det_net%d" % i] = d
    with torch.no_grad():                                         # keep box deltas small, like a trained regressor
        for i in range(0 if cls_only else heads):
            for nme in ("local_reg", "neighbor_reg1", "neighbor_reg2"):
                getattr(nets["det_net%d" % i], nme).weight.mul_(0.05)
    return args, base, ctx, nets


class C3Inference:
    """B clips [36,3,400,400], `tubes` initial tubes per clip, 3 refinement steps, batched per-class NMS (test.py:140-218).
    anchor_mode "1" .. "4": the whole anchor grid of that --anchor_mode instead (34 / 59 / 84 / 109 tubes per clip; `tubes` is not used)."""

    def __init__(self, dev, dtype, batch=4, tubes=11, seed=123, graph=True, share=None, anchor_mode=None):
        # share = another C3Inference: the same networks (weights, packed-weight caches) on other clips -- a second batch in flight
        if share is not None:
            self.args, self.base, self.ctx, self.nets = share.args, share.base, share.ctx, share.nets
        else:
            self.args, self.base, self.ctx, self.nets = build_nets(dev, seed)
        g = torch.Generator().manual_seed(seed + (1000 if share is not None else 0))
        self.x = (torch.rand(batch, 36, 3, 400, 400, generator=g) * 2 - 1).to(dev).to(dtype)
        if anchor_mode is None:
            anchors = generate_anchors()[:tubes] * 400.0
            self.tubes = [np.tile(anchors[:, None, :], (1, 3, 1)).astype(np.float32) for _ in range(batch)]
        else:
            if str(anchor_mode) not in ANCHOR_MODES:
                raise ValueError("C3Inference: anchor_mode %r" % (anchor_mode,))
            self.tubes = [(anchor_tubes(str(anchor_mode), T=3) * 400).astype(np.float32) for _ in range(batch)]
        self.batch = batch
        self.graphed = GraphedInference(self.args, self.base, self.ctx, self.nets, self.x, self.tubes) if graph else None
        if self.graphed is not None:
            self.x = self.graphed.images                      # the clips are RESIDENT in the captured step's input buffer (as bench.py's C2 loop has them)

    def eager(self):
        with torch.no_grad():
            cf = self.base(self.x)
            cx = self.ctx(cf)
            hist, _ = inference(self.args, cf, cx, self.nets, 3, self.tubes)
            return postprocess(self.args, hist)

    def step(self):
        if self.graphed is None:
            return self.eager()
        return self.finish(self.launch())

    def launch(self):
        """Enqueue the captured backbone + context + three refinement steps on the CURRENT stream; returns the history (static buffers
        the next launch() of this object overwrites).  launch() / finish() apart let a caller keep a second batch in flight."""
        with torch.no_grad():
            hist, _, _ = self.graphed(self.x)
        return hist

    def finish(self, hist):
        """Post-processing of a launched batch (thresholds, per-class NMS, the one device-to-host copy): synchronises the current stream only."""
        with torch.no_grad():
            return postprocess(self.args, hist)


def ava_clips(seed, batch):
    """`batch` synthetic AVA-shaped clips [36,3,400,400] in U(-1,1) (what ConvertFromInts(scale=2) yields), a pure function of
    the seed: rank r of a data-parallel job draws ava_clips(123 + r, ...)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(batch, 36, 3, 400, 400, generator=g) * 2 - 1


def write_padded_slots(flat, tgt, mask, inv, sel, tgts, pad, budget, num_classes, who):
    """One step's host selection into its padded host blocks (numpy, in place): `budget` slots per clip, clip b's selected rows sel[b] /
    tgts[b] first, the box pad[b] [Tl, 4] (valid for ROIAlign), all-zero targets and row weight 0 in the rest; column 0 of `flat` is the
    frame index inside the step's feature frames flattened over clips; inv[0] = 1 / (real rows x classes), the masked mean's factor."""
    Tl = flat.shape[1]
    tgt[...] = 0
    mask[...] = 0
    n_real = 0
    for b in range(len(sel)):
        n = len(sel[b])
        if n > budget:
            raise RuntimeError("%s: %d tubes selected for one clip, budget %d" % (who, n, budget))
        lo, hi = b * budget, (b + 1) * budget
        flat[lo:lo + n, :, 1:] = sel[b]
        flat[lo + n:hi, :, 1:] = pad[b]
        flat[lo:hi, :, 0] = b * Tl + np.arange(Tl, dtype=np.float32)
        tgt[lo:lo + n] = tgts[b]
        mask[lo:lo + n] = 1
        n_real += n
    inv[0] = 1.0 / (max(n_real, 1) * num_classes)


class C4TrainStep:
    """One optimisation step on `batch` AVA-shaped clips per rank (fp32): backbone + ContextNet + the max_iter = 3 heads on
    tubes of 3, 3 and 9 frames (NUM_CHUNKS 1, 1, 3), the three losses of train.py:318-331 summed over the steps
    (lambda_reg 5, lambda_nbr 1), ONE flat gradient all-reduce over ranks (step_amd.dist.allreduce_flat), ONE fused Adam
    launch that also applies 1/world and clears the gradients (step_amd.optim.FlatAdam; optimizer="sgd": step_amd.optim.FlatSGD, the
    reference's default optimizer, in its place -- same arenas, same exchange, same capture).  The reference's proposal
    selection between steps (utils/utils.py:135-423, host Python) is not part of the hot path: every step trains on the
    same `tubes_per_clip` anchor tubes, extended to the step's length."""

    def __init__(self, dev, batch=1, tubes_per_clip=5, seed=123, max_iter=3, dtype=torch.float32, capturable=False, force_exchange=False,
                 optimizer="adam", dropout=0.0, rng_seed=0, grad_wire="fp32", wire_feedback=True, max_grad_norm=None, lr_schedule=None):
        # replicas: the same weights on every rank (same init seed, then rank 0's copy is broadcast once, as DDP does);
        # `seed` only varies the rank's clips
        self.args, self.base, self.ctx, self.nets = self._build_nets(dev, max_iter, dropout)
        # dropout > 0 (the reference's recipe: 0.3): the heads' three dropout sites draw from the device-side generator (step_amd.Dropout), whose
        # offset advances inside the captured step; the state exists before any capture and is written from the host only here
        srng.manual_seed(rng_seed)
        self.rng = srng.default(dev)
        self.heads = [self.nets["det_net%d" % i] for i in range(max_iter)]
        self.mods = [self.base, self.ctx] + self.heads
        sdist.broadcast_parameters(self.mods)
        for m in self.mods:
            m.train()
        self.params = [p for m in self.mods for p in m.parameters() if p.requires_grad]
        # "adam": what the reference's scripts pick (train.py:126); "sgd": its default (train.py:123-124 with config.py:51-57's momentum
        # and weight decay).  Everything below reads the optimizer through the arena layer the two share (step_amd.optim._FlatOptimizer)
        if optimizer == "adam":
            self.opt = FlatAdam(self.params, lr=1e-5, capturable=capturable)
        elif optimizer == "sgd":
            self.opt = FlatSGD(self.params, lr=1e-5, momentum=0.9, weight_decay=1e-7, capturable=capturable)
        else:
            raise ValueError("C4TrainStep: optimizer is 'adam' or 'sgd', got %r" % (optimizer,))
        # max_grad_norm: FlatAdam / FlatSGD.step(max_grad_norm=) -- the gradient-norm clip in front of the optimizer launch, on the EXCHANGED
        # gradient; lr_schedule: a callable that builds a device scheduler on the optimizer (lambda opt: DeviceWarmupCosineLR(opt, [..])),
        # stepped in front of every optimizer step.  Both are launches of the step itself: capture() records them (in the split form, in the
        # update graph), and the replayed iteration takes neither a norm decision nor a learning rate from the host
        self.max_grad_norm = max_grad_norm
        self.sched = lr_schedule(self.opt) if lr_schedule is not None else None
        self.graph = None
        self.graph_mode = None                                   # "one" | "split" after capture()
        self._g_update = None
        # the gradient exchange runs bucket by bucket on a communication stream WHILE backward is still producing the
        # earlier layers' gradients (step_amd.dist.BucketedReducer); single-process runs issue nothing
        # (force_exchange: in a ONE-rank process group the collectives are issued all the same -- the multi-rank program on a one-GPU box)
        # grad_wire="bf16": the exchange travels as bfloat16, with error feedback unless wire_feedback=False (step_amd.dist.GradWire) -- in the
        # reducer's buckets and in the eager flat all-reduce of the split form alike.  Without an active exchange there is no wire at all.
        if grad_wire not in ("fp32", "bf16"):
            raise ValueError("C4TrainStep: grad_wire is 'fp32' or 'bf16', got %r" % (grad_wire,))
        self.force_exchange = bool(force_exchange)
        self.grad_wire = grad_wire
        self.wire = None
        if grad_wire == "bf16" and sdist._exchange_active(self.force_exchange):
            self.wire = sdist.GradWire(self.opt, "bf16", error_feedback=wire_feedback)
        self.reducer = sdist.BucketedReducer(self.opt, single_rank=self.force_exchange, wire=self.wire)
        # fp32 master weights either way; a 16-bit clip makes every activation / data gradient 16-bit (fp32 accumulate),
        # weight gradients stay fp32
        self.x = ava_clips(seed, batch).to(dev).to(dtype)
        self.batch = batch
        self.loss = None
        self._init_tubes(dev, batch, tubes_per_clip, max_iter)

    def _build_nets(self, dev, max_iter, dropout):
        """(args, BaseNet, ContextNet, nets) of this workload (a subclass with other heads builds its own)"""
        return build_nets(dev, 123, heads=max_iter, dropout=dropout)

    def _init_tubes(self, dev, batch, tubes_per_clip, max_iter):
        """the fixed tubes and targets every step trains on (a subclass that selects its tubes holds its own static state instead)"""
        anchors = torch.from_numpy(generate_anchors()[:tubes_per_clip] * 400.0).to(dev)                  # [K,4]
        K = tubes_per_clip
        self.steps = []
        for it in range(max_iter):
            Tl = 3 * self.args.NUM_CHUNKS[it + 1]
            t0 = (9 - Tl) // 2                                     # centred window of the 9 feature frames (utils.py:41-43)
            flats = []
            for b in range(batch):
                fr = (b * 9 + t0 + torch.arange(Tl, device=dev, dtype=torch.float32)).view(1, Tl, 1).expand(K, Tl, 1)
                flats.append(torch.cat([fr, anchors.view(K, 1, 4).expand(K, Tl, 4)], 2))
            self.steps.append((Tl, t0, torch.cat(flats, 0).contiguous()))
        t = torch.zeros(batch * K, 3, 66, device=dev)
        t[:, :, :4] = anchors.repeat(batch, 1).view(batch * K, 1, 4) + 4.0
        t[:, :, 4] = 1
        t[:, :, 5] = 1
        t[:, :, 6 + 7] = 1
        self.targets = t
        self.clip_of = torch.arange(batch, device=dev).repeat_interleave(K)
        self.K = K

    @staticmethod
    def _ctx_per_tube(cx, k):
        """The clip's context feature for each of its k tubes (utils.py:55-57 indexes it per tube): with the SAME number of tubes per clip this
        is a broadcast, whose backward is a fixed-order sum over the k copies -- `cx[clip_of]` is an index_select whose backward is an
        atomic index_add (24 us x 6 per step in the round-6 trace, and the one place of the step whose summation order the hardware picks)."""
        B = cx.shape[0]
        return cx.unsqueeze(1).expand(B, k, *cx.shape[1:]).reshape(B * k, *cx.shape[1:])

    def forward_backward(self, exchange=False):
        """Losses of the three steps and their gradients (into FlatAdam's gradient arena); no update.  exchange=True overlaps
        the bucketed gradient all-reduce with the backward pass and leaves the averaging factor in self.scale."""
        cf = self.base(self.x)                                    # [B,9,832,25,25]
        cx = self.ctx(cf)                                         # [B,1024,9,1,1]
        loss = 0.0
        for head, (Tl, t0, flat) in zip(self.heads, self.steps):
            pooled = self.nets["roi_net"](cf, flat)               # the frame-index column addresses frame b*9 + t of cf
            pooled = pooled.reshape(self.batch * self.K, Tl, *pooled.shape[1:])
            o = head(pooled, context_feat=self._ctx_per_tube(cx, self.K)[:, :, t0:t0 + Tl], tubes=flat, targets=self.targets)
            loss = loss + o[4].mean() + 5 * o[5].mean() + o[6].mean()
        return self._backward(loss, exchange)

    def _backward(self, loss, exchange):
        """backward into the gradient arena; exchange=True overlaps the bucketed all-reduce with it.  The averaging factor is left in self.scale."""
        if exchange:
            self.reducer.begin()
        with wgrad_into_grad():                                   # weight gradients go straight into FlatAdam's arena
            loss.backward()
        self.scale = self.reducer.finish() if exchange else 1.0
        return loss

    def _finish(self, loss):
        self._update(self.scale)
        self.loss = loss.detach()
        return self.loss

    def _update(self, grad_scale):
        """scheduler.step() (train.py:262) and optimizer.step() (train.py:348) of one iteration: the device schedule, the clip, the update
        that also clears the gradients for the next backward"""
        if self.sched is not None:
            self.sched.step()
        self.opt.step(grad_scale=grad_scale, zero_grad=True, max_grad_norm=self.max_grad_norm)

    def _eager_step(self):
        return self._finish(self.forward_backward(exchange=True))

    def step(self):
        if self.graph is not None:
            self.opt._refresh_tables()                           # lr / weight_decay of param_groups -> the device tables the captured Adam reads (schedulers keep working)
            self.graph.replay()                                  # ~800 launches (+ the bucket all-reduces of a multi-rank step), one submission
            return self._replay_tail()
        return self._eager_step()

    def _replay_tail(self):
        if self._g_update is not None:                           # split forms: forward / backward replayed, the exchange eager, the update replayed
            sdist.allreduce_flat(self.opt.flat_grad, wire=self.wire, single_rank=self.force_exchange)
            self._g_update.replay()
        # the replay re-packed the weights at its start and Adam changed them at its end: any eager use of the modules between
        # replays (validation) must see its packed-weight caches as stale
        torch.autograd.graph.increment_version(self.params)
        return self.loss

    @staticmethod
    def _world():
        dd = torch.distributed
        return dd.get_world_size() if (dd.is_available() and dd.is_initialized()) else 1

    def _record(self, fn, pool=None):
        """fn() recorded (not executed) as a graph of its own, in `pool` or a fresh one"""
        # with a live process group its watchdog / heartbeat threads may touch the runtime while this thread records: only THIS thread's
        # calls are checked against the capture
        kw = {"capture_error_mode": "thread_local"} if self.reducer.active else {}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool, **kw):
            fn()
        return g

    def _record_update(self, pool=None):
        """the update as a graph of its own, replayed behind ONE eager flat all-reduce (nothing of the process group is recorded)"""
        scale = 1.0 / self._world()
        return self._record(lambda: self._update(scale), pool)

    def _warm(self, warmup):
        dev = self.x.device
        cur = torch.cuda.current_stream(dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._eager_step()
        cur.wait_stream(s)
        torch.cuda.synchronize(dev)

    def capture(self, warmup=3, mode="auto"):
        """Capture the WHOLE step (forward, backward with the side-stream weight gradients, the gradient exchange, weight re-pack, Adam)
        in one HIP graph; step() then replays it.  The shapes of this step are static (fixed tubes per clip), every scalar that
        changes between steps lives on the device (FlatAdam(capturable=True): step counter), and nothing on the path synchronises with
        the host -- with 16-bit activations the eager step is bound by the host issuing ~800 launches, not by the GPU.

        With a process group (the reference's step is one optimizer.step() per iteration over all devices, train.py:142-148,257-348) the
        N > 1 step is the SAME program as the N = 1 step: mode "one" records the bucket all-reduces on the communication stream
        inside the graph (RCCL collectives are stream-ordered and capturable; ProcessGroupNCCL issues them on its own stream, forked
        from and joined to the capturing stream by events, and keeps captured work off its watchdog) -- the overlap of the exchange with
        backward is part of the replayed graph.  Mode "split" is the fallback where the collectives cannot be recorded (a gloo group;
        an RCCL build that refuses capture): graph 1 = forward + backward into the gradient arena, the exchange eager as ONE flat
        all-reduce, graph 2 = re-pack + Adam.  "auto" = "one" on nccl, falling back to "split" if the capture raises.
        Runs `warmup` eager steps first (caches, pack tables, workspaces, the communicator); the captured step itself is recorded,
        not executed."""
        if not self.opt.capturable:
            raise RuntimeError("C4TrainStep.capture: build the workload with capturable=True (device-side optimizer step counter)")
        import gc
        dd = torch.distributed
        grouped = self.reducer.active
        backend = dd.get_backend() if (dd.is_available() and dd.is_initialized()) else None
        if mode == "auto":
            # with a process group: "split" -- nothing of the group is recorded, so its watchdog thread cannot collide with the capture
            # (the "one" form's guard is a pause, and the failure is a process abort no fallback can catch).  "one" with
            # collectives stays available on request; it replays bit-identically (tests/test_gpu_ddp.py) and measured 13.55 ms against
            # 13.47 ms split on the one-GPU box -- nothing is lost by the safe default until the form has run on real multi-GPU hardware.
            mode = "one" if not grouped else "split"
        if mode not in ("one", "split"):
            raise ValueError("C4TrainStep.capture: mode is 'auto', 'one' or 'split'")
        if mode == "one" and grouped and backend != "nccl":
            raise RuntimeError("C4TrainStep.capture(mode='one'): only RCCL ('nccl') collectives can be recorded in a HIP graph; use mode='split'")
        gc.collect()                                             # (torch.cuda.graph collects too: dead nets must not drop out of the re-pack table mid-capture)
        # at least TWO eager steps: the second one is the first that re-packs every weight in one launch (backbone._repack_all) and builds
        # that launch's device tables with host -> device copies, which a capture cannot record (seen in round 6 with warmup = 1:
        # hipErrorStreamCaptureUnsupported in both capture modes)
        self._warm(max(int(warmup), 2))
        dev = self.x.device
        if grouped and backend == "nccl" and mode == "one":
            # OPT-IN form.  The process group's watchdog thread polls the completion events of the collectives the warm-up steps issued
            # (every ~100 ms); if it still holds some when the capture begins it queries them while the group's internal stream is
            # capturing, HIP answers hipErrorCapturedEvent and the watchdog ABORTS the process (no exception to catch).  Round 5 guarded
            # this with a pause (1 abort in 8 runs without, 0 in 6 with); round 6 tried to replace the pause by a deterministic drain read
            # from the group's flight recorder -- the recorder's own event queries made it worse (abort inside a 30-capture loop,
            # gpurun_out of call c2) -- and no other API exposes the watchdog's list.  So the pause stays for callers who ask for "one"
            # explicitly, and "auto" no longer picks this form with a live process group (see above).
            import os
            import time
            torch.cuda.synchronize(dev)
            time.sleep(float(os.environ.get("STEP_PG_DRAIN_S", "1.0")))
        if mode == "one":
            try:
                self.graph, self.graph_mode, self._g_update = self._record(self._eager_step), "one", None
            except RuntimeError as e:
                if not grouped:
                    raise
                import warnings
                warnings.warn("C4TrainStep.capture: recording the gradient exchange failed (%s); falling back to the split form" % (str(e).splitlines()[0],))
                torch.cuda.synchronize(dev)
                self.reducer._armed = False
                wgrad.STATE.disarm()
                wgrad.STATE.sync()
                self.opt.zero_grad()
                mode = "split"
        if mode == "split":
            def fwd_bwd():
                self.loss = self.forward_backward(exchange=False).detach()
            g1 = self._record(fwd_bwd)
            self.graph, self._g_update, self.graph_mode = g1, self._record_update(), "split"       # (two graphs, two pools)
        # host-side caches now carry the version stamps of a step whose kernels only run on replay: make them stale again for
        # any eager use of the modules after this point
        torch.autograd.graph.increment_version(self.params)
        return self


class C4SelectTrainStep(C4TrainStep):
    """The reference's whole training iteration (train.py:257-348), proposal selection included: backbone + ContextNet with
    gradients; an eval-mode, no-grad inference() over the first max_iter-1 steps to get the refined tubes; then for every
    step train_select() (step_amd.selection: the reference's sampling, same RNG streams) picks positives / negatives among
    them, ROIAlign pools the selected tubes, the step's head returns the three losses; one backward, one flat gradient
    all-reduce, one fused Adam launch.  `targets`: 2 ground-truth tubes per clip with 3 positive classes each.

    Three forms of the same iteration:
      step()          eager, ragged: every head sees exactly the selected tubes (shapes change from iteration to iteration)
      step_padded()   eager, STATIC shapes: every clip's selection is padded to `budget` slots (max_pos_num x (1 + neg_ratio) = 15); padded
                      slots carry a copy of the clip's first initial tube, all-zero targets and row weight 0 -- they receive exactly zero loss
                      and zero gradient (the classification loss is the masked mean over the real rows, the regression losses are masked by
                      their flags already)
      capture()       the padded form replayed as HIP graphs: graph F = backbone + ContextNet forward (with gradients)
                      + the no-grad inference; HOST: train_select on the inference's static outputs (one launch + one small copy per step,
                      then the draws from `random` / `numpy.random` in the reference's order) writes the selection into static device
                      buffers; graph B = ROIAlign + the three heads + losses + backward + re-pack + Adam (with a process group: B stops after
                      backward, ONE eager flat all-reduce, graph U = re-pack + Adam -- the split form, nothing of the group is recorded).
                      Same kernels on the same buffers as step_padded(): bit-identical trajectory (tests/test_gpu_graph_step.py).

    selection="device" (opt-in; "host" is the default and the form that reproduces the reference's draws): the padded forms select on the
    device instead (step_amd.selection.DeviceSelector: step_select_prepare + step_select_train per step, draws from `self.rng`, one offset
    per step) -- no copy, no host work between the first launch of the iteration and the last, so capture() records front, selection and
    back as ONE graph ("select-one"; with a process group one graph up to the backward, the eager flat all-reduce, the update graph:
    "select-one-split").  The ragged step() keeps the host selection -- before capture(), step() of a selection="device" workload is
    therefore the HOST form; `selection_ran` names the selection of the last iteration, and a caller that wants the device selection
    uncaptured calls step_padded() (train_step_amd.py --select-device --no-graph does).

    augment=<step_amd.DeviceTubeAugmentation> (opt-in, selection="device" only): the padded forms start from uint8 frames.  `stage`
    [B,T,Hs,Ws,3] (src_size) is the iteration's input -- the captured one -- and the front begins with the planner, the noise fill and
    step_clip_augment_u8, which write the clip `x` AND the ground truths the selector reads (`d_gt`, `d_gt_count`: the tubes the crop kept,
    in pixels of the network's resolution), both from the same draws; `d_gt_in` / `d_gt_count_in` hold the loader's percent boxes.  Two
    more offsets of the generator per iteration.  An augmentation built with rng=None draws from the workload's generator.

    proposals=K (opt-in, selection="device" only): the initial tubes are a person detector's PROPOSALS, whose number changes from key frame
    to key frame, instead of the anchor grid (train.py:85-86, data/ava.py:320-358).  A clip owns K slots, the first `d_count[b]` real, the
    others the whole frame; `d_prop_in` [B,K,T,4] (percent) and `d_prop_count` [B] hold what the loader read -- synthetic here, drawn from
    the seed: counts from 0 to K, with B > 1 at least one clip at 0, which falls back to `d_fill`, the first min(34, K) anchors.  With
    augment= the front's planner transforms them with the frames (apply(tubes=...): the step-1 candidates and their count are written by the
    iteration itself); without, they are scaled once.  The no-grad inference runs over B * K slots with the counts, the selector gets
    clip_count.  set_proposals(list of [n_i,T,4] percent arrays) feeds the next iteration's proposals into the static buffers: no
    recapture.  The ragged step() runs the host selection on the real ragged lists.

    temporal_mode="predict" | "extrapolate" | "mean" (config.py:92; every shipped script passes "predict"): how the tubes grow from one chunk
    to three, in the no-grad inference and in the selection alike.  Outside "predict" nobody reads the heads' neighbour regressions for the
    next step and no neighbour targets are written; both selections handle all three modes, so selection="device" stays ONE graph."""

    def __init__(self, dev, batch=1, seed=123, dtype=torch.float32, tubes_per_clip=34, capturable=False, force_exchange=False, budget=None,
                 optimizer="adam", dropout=0.0, rng_seed=0, selection="host", grad_wire="fp32", wire_feedback=True, max_grad_norm=None,
                 lr_schedule=None, augment=None, src_size=(256, 340), proposals=None, temporal_mode="predict"):
        if temporal_mode not in DeviceSelector.ALL_MODES:
            raise ValueError("C4SelectTrainStep: temporal_mode is one of %r, got %r" % (DeviceSelector.ALL_MODES, temporal_mode))
        if selection not in ("host", "device"):
            raise ValueError("C4SelectTrainStep: selection is 'host' or 'device', got %r" % (selection,))
        if proposals is not None and (selection != "device" or int(proposals) < 1):
            raise ValueError("C4SelectTrainStep: proposals=K (K >= 1 slots per clip) needs selection='device' (the host selection keeps its ragged form)")
        if augment is not None and selection != "device":
            raise ValueError("C4SelectTrainStep: augment= needs selection='device' (the host selection reads ground truths the device cannot hand it)")
        super().__init__(dev, batch=batch, tubes_per_clip=5, seed=seed, max_iter=3, dtype=dtype, capturable=capturable, force_exchange=force_exchange,
                         optimizer=optimizer, dropout=dropout, rng_seed=rng_seed, grad_wire=grad_wire, wire_feedback=wire_feedback,
                         max_grad_norm=max_grad_norm, lr_schedule=lr_schedule)
        self.args.temporal_mode = temporal_mode                  # (read by the no-grad inference and by both selections, nowhere in the networks)
        rs = np.random.RandomState(seed)
        anchors = (generate_anchors()[:tubes_per_clip] * 400.0).astype(np.float32)
        self.init_tubes = [np.tile(anchors[:, None, :], (1, 3, 1)) for _ in range(batch)]
        self.gt = []
        for _ in range(batch):
            t = np.zeros((2, 3, 4 + 60), np.float32)
            for g_ in range(2):
                box = anchors[rs.randint(0, len(anchors))] + rs.uniform(-20, 20, 4).astype(np.float32)
                for c in range(3):
                    t[g_, c, :4] = box + rs.uniform(-5, 5, 4).astype(np.float32)
                t[g_, :, 4 + rs.randint(0, 60, 3)] = 1
            self.gt.append(t)
        self.proposals = None if proposals is None else int(proposals)
        if self.proposals is not None:
            K_, W_, H_ = self.proposals, float(self.args.image_size[0]), float(self.args.image_size[1])
            self.fill = generate_anchors()[:min(34, K_)].astype(np.float32)                      # percent boxes: the fallback of data/ava.py:342-358
            cnt = rs.randint(1, K_ + 1, batch)
            if batch > 1:
                cnt[-1] = 0
            gt_pct = [t[:, :, :4] / np.array([W_, H_, W_, H_], np.float32) for t in self.gt]
            props = []
            for b in range(batch):                               # half of a clip's proposals sit on its ground truths, the others anywhere
                p = np.zeros((int(cnt[b]), 3, 4), np.float32)
                for j in range(int(cnt[b])):
                    if j % 2 == 0:
                        box = gt_pct[b][(j // 2) % 2, 1] + rs.uniform(-0.03, 0.03, 4)
                    else:
                        xy = rs.uniform(0.0, 0.6, 2)
                        box = np.concatenate([xy, xy + rs.uniform(0.15, 0.35, 2)])
                    p[j] = box[None, :] + rs.uniform(-0.01, 0.01, (3, 4))
                props.append(p)
            self._props = props
            self.init_tubes = self._scaled(props)
        self.selection = selection
        self.selection_ran = None                                # "host" | "device": the selection of the LAST iteration (step() before capture() is the ragged form: host)
        self._selected = []
        a = self.args
        self.budget = int(budget or a.max_pos_num * (1 + a.neg_ratio))
        # static state of the padded form
        K = batch * self.budget
        if self.proposals is None:
            self.flat0, self.nums0 = _flat_tubes(self.init_tubes, dev)
            self.d_count = None
        else:
            self.flat0, self.d_count = pad_tubes(self.init_tubes, self.proposals, dev, *self.args.image_size[:2])
            self.nums0 = [self.proposals] * batch
        self.clip_of0 = torch.as_tensor(np.repeat(np.arange(batch), self.nums0), device=dev)
        self.clip_of_pad = torch.arange(batch, device=dev).repeat_interleave(self.budget)
        self.s_flat, self.s_tgt, self.s_mask, self.s_inv = [], [], [], []
        self.h_flat, self.h_tgt, self.h_mask, self.h_inv = [], [], [], []
        self.pad = []                                            # per step [B, Tl, 4]: the clip's first initial tube, a valid box for the padded slots' ROIAlign
        for i in range(1, a.max_iter + 1):
            Tl = a.NUM_CHUNKS[i] * a.T                           # (the last step's tubes are 3 chunks long)
            if self.proposals is None:
                self.pad.append(np.stack([np.tile(np.asarray(t[0], np.float32), (Tl // t.shape[1] + 1, 1))[:Tl] for t in self.init_tubes]))
            else:                                                # (a clip's first proposal changes under the graph: the first anchor, the anchor form's pad)
                wh = np.array([a.image_size[0], a.image_size[1]] * 2, np.float32)
                self.pad.append(np.tile(self.fill[0] * wh, (batch, Tl, 1)))
            for dst, host, shape in ((self.s_flat, self.h_flat, (K, Tl, 5)), (self.s_tgt, self.h_tgt, (K, 3, 6 + a.num_classes)),
                                     (self.s_mask, self.h_mask, (K, 1)), (self.s_inv, self.h_inv, (1,))):
                dst.append(torch.zeros(shape, device=dev) if selection == "host" else None)     # (device: the selector's own buffers, below)
                if selection == "host":
                    host.append(torch.zeros(shape).pin_memory())
        if selection == "device":
            # everything the selection reads is resident: ground truths, the initial tubes (step 1's candidates), the padded slots' box
            self.selector = DeviceSelector(a, batch, self.budget, dev, self.rng, dynamic_gt=augment is not None,
                                           temporal_modes=DeviceSelector.ALL_MODES)
            self.d_gt = torch.from_numpy(np.stack(self.gt)).to(dev)
            self.d_gt_count = torch.full((batch,), self.gt[0].shape[0], dtype=torch.int32, device=dev)
            self.d_init = self.flat0[:, :, 1:].float().contiguous()
            self.d_clip_start = torch.as_tensor(np.concatenate(([0], np.cumsum(self.nums0))).astype(np.int32), device=dev)
            self.d_pad = []
            for i in range(1, a.max_iter + 1):
                self.d_pad.append(torch.from_numpy(self.pad[i - 1]).to(dev))
                self.s_flat[i - 1], self.s_tgt[i - 1], self.s_mask[i - 1], self.s_inv[i - 1] = self.selector.out[i][:4]
        self.augment = augment
        if augment is not None:
            _, T, _, H, W = self.x.shape
            if tuple(augment.size) != (W, H):
                raise ValueError("C4SelectTrainStep: the augmentation resizes to %r, the clips are %r" % (tuple(augment.size), (W, H)))
            if augment.rng is None:
                augment.rng = self.rng
            Hs, Ws = (int(v) for v in src_size)
            g_ = torch.Generator().manual_seed(seed + 7)
            self.stage = torch.randint(0, 256, (batch, T, Hs, Ws, 3), dtype=torch.uint8, generator=g_).to(dev)
            whwh = torch.tensor([a.image_size[0], a.image_size[1]] * 2, dtype=torch.float32, device=dev)
            self.d_gt_in = self.d_gt.clone()                     # what the loader reads: percent boxes (data/ava.py:283-296)
            self.d_gt_in[..., :4] = (self.d_gt[..., :4] / whwh).clamp_(0.0, 1.0)
            self.d_gt_count_in = self.d_gt_count.clone()
        if self.proposals is not None:
            self.d_prop_in = torch.zeros((batch, self.proposals, 3, 4), device=dev)
            self.d_prop_count = torch.zeros(batch, dtype=torch.int32, device=dev)
            self.d_fill = torch.from_numpy(self.fill).to(dev)
            self.d_init_slots = self.d_init.view(batch, self.proposals, 3, 4)     # (what the planner writes: the selector's step-1 candidates)
            self.set_proposals(self._props)
        self._gF = self._gB = None
        self._front = None

    @property
    def selected(self):
        """tubes selected per step and clip in the last iteration; with the device selection this reads `counts` (and synchronises)"""
        if self._selected is None:
            return [[int(v) for v in c.sum(axis=1)] for c in self.select_counts()]
        return self._selected

    @selected.setter
    def selected(self, value):
        self._selected = value

    def _scaled(self, props):
        """percent proposals per clip -> the ragged pixel tubes of the form without augmentation: scale_tubes_abs; a clip without any gets
        the fill (data/ava.py:342-362)"""
        W, H = float(self.args.image_size[0]), float(self.args.image_size[1])
        out = []
        for p in props:
            p = np.asarray(p, np.float64).reshape(-1, 3, 4)
            if p.shape[0] == 0:
                p = np.repeat(self.fill.astype(np.float64)[:, None, :], 3, axis=1)
            out.append((np.minimum(np.maximum(p, 0.0), 1.0) * np.array([W, H, W, H])).astype(np.float32))
        return out

    def set_proposals(self, props):
        """props: per clip an array [n_i,T,4] of percent boxes, 0 <= n_i <= K (an empty clip falls back to the fill): the NEXT iteration's
        proposals, written into the static buffers the eager and the captured forms read -- no recapture.  With augment= they go to the
        planner's inputs; without, they are scaled here and go to the slots themselves."""
        if self.proposals is None:
            raise RuntimeError("C4SelectTrainStep: set_proposals needs a workload built with proposals=K")
        K, B = self.proposals, self.batch
        props = [np.asarray(p, np.float32).reshape(-1, 3, 4) for p in props]
        if len(props) != B or any(p.shape[0] > K for p in props):
            raise ValueError("C4SelectTrainStep: set_proposals takes %d clips of at most %d proposals" % (B, K))
        self._props = props
        self.init_tubes = self._scaled(props)
        host = np.zeros((B, K, 3, 4), np.float32)
        for b, p in enumerate(props):
            host[b, :p.shape[0]] = p
        self.d_prop_in.copy_(torch.from_numpy(host))
        self.d_prop_count.copy_(torch.tensor([p.shape[0] for p in props], dtype=torch.int32))
        if self.augment is None:
            flat, count = pad_tubes(self.init_tubes, K, "cpu", *self.args.image_size[:2])
            self.flat0.copy_(flat)
            self.d_count.copy_(count)
            self.d_init.copy_(self.flat0[:, :, 1:])

    def select_counts(self):
        """device selection: [max_iter, B, 2] (positives, negatives) of the last iteration, on the host; synchronises"""
        return np.stack([self.selector.out[i][4].cpu().numpy() for i in range(1, self.args.max_iter + 1)])

    # ---- the ragged eager iteration (the reference's program, shapes follow the selection)
    def step(self):
        if self._gF is not None:
            return self._replay()
        if self.augment is not None:
            raise RuntimeError("C4SelectTrainStep: the ragged step() selects on the host and knows no augmentation; use step_padded() or capture()")
        a = self.args
        cf = self.base(self.x)
        cx = self.ctx(cf)
        for m in self.mods:
            m.eval()
        with torch.no_grad():
            history, _ = inference(a, cf.detach(), cx.detach(), self.nets, a.max_iter - 1, self.init_tubes)
        for m in self.mods:
            m.train()
        loss = 0.0
        self.selected = []
        for i in range(1, a.max_iter + 1):
            chunks, max_chunks = a.NUM_CHUNKS[i], a.NUM_CHUNKS[a.max_iter]
            t0 = int((max_chunks - chunks) / 2) * a.T
            Tl = chunks * a.T
            sel, tgt = train_select(i, history[i - 2] if i > 1 else None, self.gt, self.init_tubes, a)
            self.selection_ran = "host"
            self.selected.append([len(s_) for s_ in sel])
            flat, nums = _flat_tubes(sel, cf.device)
            targets = torch.from_numpy(np.concatenate(tgt, axis=0)).to(cf.device)
            clip_of = torch.as_tensor(np.repeat(np.arange(len(nums)), nums), device=cf.device)
            pooled = self.nets["roi_net"](cf[:, t0:t0 + Tl], flat)
            pooled = pooled.reshape(flat.shape[0], Tl, *pooled.shape[1:])
            o = self.heads[i - 1](pooled, context_feat=cx[clip_of][:, :, t0:t0 + Tl], tubes=flat, targets=targets)
            loss = loss + o[4].mean() + a.lambda_reg * o[5].mean() + a.lambda_neighbor * o[6].mean()
        return self._finish(self._backward(loss, True))

    # ---- the padded iteration in its three parts
    def _front_part(self):
        """backbone + ContextNet (with gradients) and the no-grad, eval-mode inference over the first max_iter - 1 steps (train.py:266-272)"""
        a = self.args
        if self.augment is not None:                            # decisions, noise, pixels and boxes of this iteration, from the same two offsets
            if self.proposals is None:
                self.augment.apply(self.stage, self.d_gt_in, self.d_gt_count_in, out=self.x, gt_out=self.d_gt, gt_count_out=self.d_gt_count)
            else:                                               # ... and the proposals: the step-1 candidates, their count, the inference's slots
                self.augment.apply(self.stage, self.d_gt_in, self.d_gt_count_in, out=self.x, gt_out=self.d_gt, gt_count_out=self.d_gt_count,
                                   tubes=self.d_prop_in, tube_count=self.d_prop_count, fill=self.d_fill, tubes_out=self.d_init_slots,
                                   tube_count_out=self.d_count)
                self.flat0[:, :, 1:].copy_(self.d_init)
        cf = self.base(self.x)
        cx = self.ctx(cf)
        for m in self.mods:
            m.eval()
        with torch.no_grad():
            history, _ = inference_flat(a, cf.detach(), cx.detach(), self.nets, a.max_iter - 1, self.flat0, self.nums0, self.clip_of0, want_classes=False,
                                        counts=self.d_count)
        for m in self.mods:
            m.train()
        return cf, cx, history

    def _select_part(self, history):
        """HOST (default): train_select per step on the inference's outputs, padded to `budget` slots per clip, into the static device buffers;
        selection="device": the same rows chosen and written by DeviceSelector, stream-ordered, with no copy either way"""
        a = self.args
        if self.selection == "device":                          # DEVICE: two launches + their finishing kernel per step, nothing comes back
            self._selected = None
            self.selection_ran = "device"
            for i in range(1, a.max_iter + 1):
                self.selector.select(i, history[i - 2] if i > 1 else None, self.d_gt, self.d_gt_count, self.d_init, self.d_clip_start,
                                     self.d_pad[i - 1], max_tubes=max(self.nums0), clip_count=self.d_count)
            return
        self.selected = []
        self.selection_ran = "host"
        for i in range(1, a.max_iter + 1):
            sel, tgt = train_select(i, history[i - 2] if i > 1 else None, self.gt, self.init_tubes, a)
            self.selected.append([len(s_) for s_ in sel])
            # ONE set of pinned blocks: from step 2 on train_select reads the front's outputs on the host, a copy that is stream-ordered behind
            # every earlier copy out of these blocks (step 1's block was copied ahead of that read in the iteration before)
            blocks = (self.h_flat[i - 1], self.h_tgt[i - 1], self.h_mask[i - 1], self.h_inv[i - 1])
            write_padded_slots(*(h.numpy() for h in blocks), sel, tgt, self.pad[i - 1], self.budget, a.num_classes, "C4SelectTrainStep")
            for dst, src in zip((self.s_flat[i - 1], self.s_tgt[i - 1], self.s_mask[i - 1], self.s_inv[i - 1]), blocks):
                dst.copy_(src, non_blocking=True)

    def _loss_part(self, cf, cx):
        a = self.args
        loss = 0.0
        K = self.batch * self.budget
        for i in range(1, a.max_iter + 1):
            chunks, max_chunks = a.NUM_CHUNKS[i], a.NUM_CHUNKS[a.max_iter]
            t0 = int((max_chunks - chunks) / 2) * a.T
            Tl = chunks * a.T
            flat = self.s_flat[i - 1]
            pooled = self.nets["roi_net"](cf[:, t0:t0 + Tl], flat)
            pooled = pooled.reshape(K, Tl, *pooled.shape[1:])
            o = self.heads[i - 1](pooled, context_feat=self._ctx_per_tube(cx, self.budget)[:, :, t0:t0 + Tl], tubes=flat, targets=self.s_tgt[i - 1])
            # o[4]: the element-wise classification loss [K * classes]; the reference's .mean() runs over the REAL rows only
            lcls = (o[4].view(K, -1) * self.s_mask[i - 1]).sum() * self.s_inv[i - 1][0]
            loss = loss + lcls + a.lambda_reg * o[5].mean() + a.lambda_neighbor * o[6].mean()
        return loss

    def _back_part(self, cf, cx, update=True):
        loss = self._loss_part(cf, cx)
        self._backward(loss, update)                             # (split form: the exchange is eager, between the graphs)
        if update:
            return self._finish(loss)
        self.loss = loss.detach()
        return self.loss

    def step_padded(self):
        cf, cx, hist = self._front_part()
        self._select_part(hist)
        return self._back_part(cf, cx)

    def _eager_step(self):                                       # (what bench.py instruments for the per-kernel roofline)
        return self.step_padded()

    def capture(self, warmup=2, mode="auto"):
        """See the class docstring.  With a process group the update is a graph of its own behind ONE eager flat all-reduce (the split
        form of C4TrainStep.capture: nothing of the group is recorded)."""
        if not self.opt.capturable:
            raise RuntimeError("C4SelectTrainStep.capture: build the workload with capturable=True")
        import gc
        grouped = self.reducer.active
        gc.collect()
        self._warm(max(int(warmup), 2))
        dev = self.x.device
        if self.selection == "device":
            # nothing between the iteration's first launch and its last needs the host: front, selection and back are ONE recording
            front = []                                           # (the front's outputs stay alive while the update is recorded into the same pool)

            def whole():
                front[:] = self._front_part()
                self._select_part(front[2])
                self._back_part(front[0], front[1], update=not grouped)
            gF, gB, form = self._record(whole), None, "select-one"
        else:
            def front_part():
                self._front = self._front_part()
            gF, form = self._record(front_part), "select"
            cf, cx, hist = self._front
            gF.replay()                                          # (a capture records, it does not run: give the selection real predictions to read)
            torch.cuda.synchronize(dev)
            import random
            rs_py, rs_np = random.getstate(), np.random.get_state()  # this selection trains nothing: it must not consume draws of the reference's RNG streams
            self._select_part(hist)
            random.setstate(rs_py)
            np.random.set_state(rs_np)
            torch.cuda.synchronize(dev)
            gB = self._record(lambda: self._back_part(cf, cx, update=not grouped), gF.pool())
        gU = self._record_update(gF.pool()) if grouped else None     # (the select forms share the front graph's pool)
        self._gF, self._gB, self._g_update = gF, gB, gU
        self.graph, self.graph_mode = gF, form + ("-split" if grouped else "")
        torch.autograd.graph.increment_version(self.params)
        return self

    def _replay(self):
        self.opt._refresh_tables()
        self._gF.replay()
        if self._gB is not None:                                 # (device selection: the one graph holds all three parts)
            self._select_part(self._front[2])                    # host: reads the inference's static outputs (one small copy per step)
            self._gB.replay()
        return self._replay_tail()


class C4ClsTrainStep(C4TrainStep):
    """The reference's classification pre-training iteration (train_cls.py:230-322, stage 1 of its two-stage recipe: scripts/train_cls.sh
    writes the checkpoint scripts/train_step.sh loads as --pretrain_path): backbone + ContextNet, ONE cls_only head on tubes of T = 9 frames
    (NUM_CHUNKS 1), trained on boxes sampled around the ground truths -- sample_anchors in the loader (data/ava_cls.py:200-261, one positive
    and three negatives per box), then select_proposals per clip (train_cls.py:263-291) -- with the classification loss alone; one backward,
    one flat gradient exchange, one fused optimizer launch.  `gt`: 2 ground-truth boxes per clip on one frame, 3 positive classes each.

    The three forms of C4SelectTrainStep:
      step()          eager, ragged: the reference's program -- selection.sample_anchors and selection.cls_select on the host (the reference's
                      `random` / `numpy.random` streams), the head sees exactly the selected tubes, loss.mean()
      step_padded()   eager, STATIC shapes: 20 slots per clip (5 positives x (1 + 3)); padded slots hold the clip's first ground-truth box,
                      all-zero targets and row weight 0, the loss is the masked sum over the real rows times 1 / (rows * classes); the context
                      feature goes per tube as a broadcast (no .item() per tube, train_cls.py:307-308)
      capture()       the padded form as ONE graph (C4TrainStep.capture: with a process group the split form around one eager flat
                      all-reduce).  selection="host": sampling and selection read no network output, so step() draws them BEFORE the replay,
                      into pinned blocks that are copied into the graph's static buffers; selection="device" (opt-in): step_anchor_sample and
                      step_select_train (selection.DeviceClsSelector, draws from `self.rng`, two offsets per iteration) are inside the graph.
    As in C4SelectTrainStep, step() before capture() is the ragged HOST form whatever `selection` says; `selection_ran` names the last one."""
    BUDGET = DeviceClsSelector.BUDGET

    def __init__(self, dev, batch=1, seed=123, dtype=torch.float32, capturable=False, force_exchange=False, optimizer="adam", dropout=0.0,
                 rng_seed=0, selection="host", grad_wire="fp32", wire_feedback=True, max_grad_norm=None, lr_schedule=None):
        if selection not in ("host", "device"):
            raise ValueError("C4ClsTrainStep: selection is 'host' or 'device', got %r" % (selection,))
        self.selection = selection
        self.selection_ran = None
        self._seed = seed
        super().__init__(dev, batch=batch, tubes_per_clip=0, seed=seed, max_iter=1, dtype=dtype, capturable=capturable, force_exchange=force_exchange,
                         optimizer=optimizer, dropout=dropout, rng_seed=rng_seed, grad_wire=grad_wire, wire_feedback=wire_feedback,
                         max_grad_norm=max_grad_norm, lr_schedule=lr_schedule)

    def _build_nets(self, dev, max_iter, dropout):
        return build_nets(dev, 123, heads=1, cls_only=True, dropout=dropout, T=9, max_iter=1, NUM_CHUNKS={1: 1})     # scripts/train_cls.sh: --T 9

    def _init_tubes(self, dev, batch, tubes_per_clip, max_iter):
        a = self.args
        rs = np.random.RandomState(self._seed)
        anchors = (generate_anchors()[:34] * 400.0).astype(np.float32)
        self.gt = []
        for _ in range(batch):
            t = np.zeros((2, 1, 4 + a.num_classes), np.float32)
            for g_ in range(2):
                t[g_, 0, :4] = np.clip(anchors[rs.randint(0, len(anchors))] + rs.uniform(-20, 20, 4).astype(np.float32), 0, 400)
                t[g_, 0, 4 + rs.randint(0, a.num_classes, 3)] = 1
            self.gt.append(t)
        self.budget = self.BUDGET
        K, Tl = batch * self.budget, a.T * a.NUM_CHUNKS[1]
        self.Tl = Tl
        self._selected = []
        self.pad = np.stack([np.tile(t[0, 0, :4], (Tl, 1)) for t in self.gt]).astype(np.float32)       # a valid box for the padded slots' ROIAlign
        if self.selection == "device":
            self.selector = DeviceClsSelector(a, batch, 2, dev, self.rng)
            self.d_gt = torch.from_numpy(np.stack(self.gt)).to(dev)
            self.d_gt_count = torch.full((batch,), 2, dtype=torch.int32, device=dev)
            self.d_pad = torch.from_numpy(self.pad).to(dev)
            self.s_flat, self.s_tgt, self.s_mask, self.s_inv = self.selector.out[:4]
        else:
            shapes = ((K, Tl, 5), (K, 3, 6 + a.num_classes), (K, 1), (1,))
            self.s_flat, self.s_tgt, self.s_mask, self.s_inv = (torch.zeros(sh, device=dev) for sh in shapes)
            # TWO sets of pinned blocks, used in turn: the host fills the next iteration's set while the copies of the last one may still be
            # queued behind a replay; a set is written again only after the event behind its copies has passed
            self._pinned = [tuple(torch.zeros(sh).pin_memory() for sh in shapes) for _ in range(2)]
            self._pinned_free = [None, None]
            self._turn = 0
            for hf, _, _, _ in self._pinned:
                for b in range(batch):                            # (valid boxes before the first selection is copied in)
                    hf[b * self.budget:(b + 1) * self.budget, :, 1:] = torch.from_numpy(self.pad[b])
                    hf[b * self.budget:(b + 1) * self.budget, :, 0] = b * Tl + torch.arange(Tl, dtype=torch.float32)
            self.s_flat.copy_(self._pinned[0][0])

    @property
    def selected(self):
        """rows selected per clip in the last iteration; with the device selection this reads `counts` (and synchronises)"""
        if self._selected is None:
            return [int(v) for v in self.select_counts().sum(axis=1)]
        return self._selected

    def select_counts(self):
        """device selection: [B, 2] (positives, negatives) of the last iteration, on the host; synchronises"""
        return self.selector.out[4].cpu().numpy()

    # ---- the host's sampling and selection (the reference's loader, then its training loop)
    def _host_selection(self):
        a = self.args
        W, H = float(a.image_size[0]), float(a.image_size[1])
        whwh = np.array([W, H, W, H], np.float64)
        tubes = []
        for t in self.gt:                                        # data/ava_cls.py:351-357, one clip after the other
            boxes = sample_anchors(t[:, 0, :4].astype(np.float64) / whwh, neg_ratio=3, mode="train")
            tubes.append(np.tile((boxes * whwh).astype(np.float32)[:, None, :], (1, self.Tl, 1)))
        sel, tgt = cls_select(self.gt, tubes, a)
        self._selected = [len(s_) for s_ in sel]
        self.selection_ran = "host"
        self.last_selection = (sel, tgt)
        return sel, tgt

    def _select_host_padded(self):
        """the host selection into the pinned blocks, then four stream-ordered copies into the static buffers"""
        a = self.args
        sel, tgt = self._host_selection()
        k = self._turn
        self._turn = 1 - k
        if self._pinned_free[k] is not None:
            self._pinned_free[k].synchronize()
        blocks = self._pinned[k]
        write_padded_slots(*(h.numpy() for h in blocks), sel, tgt, self.pad, self.budget, a.num_classes, "C4ClsTrainStep")
        for dst, src in zip((self.s_flat, self.s_tgt, self.s_mask, self.s_inv), blocks):
            dst.copy_(src, non_blocking=True)
        if self.s_flat.is_cuda:
            self._pinned_free[k] = torch.cuda.Event()
            self._pinned_free[k].record()

    # ---- the ragged eager iteration (the reference's program)
    def step(self):
        if self.graph is not None:
            if self.selection == "host":
                self._select_host_padded()                       # before the replay: the one graph reads the static buffers
            return super().step()
        sel, tgt = self._host_selection()
        cf = self.base(self.x)
        cx = self.ctx(cf)
        flat, nums = _flat_tubes(sel, cf.device)
        targets = torch.from_numpy(np.concatenate(tgt, axis=0)).to(cf.device)
        clip_of = torch.as_tensor(np.repeat(np.arange(len(nums)), nums), device=cf.device)
        pooled = self.nets["roi_net"](cf, flat)
        pooled = pooled.reshape(flat.shape[0], self.Tl, *pooled.shape[1:])
        o = self.heads[0](pooled, context_feat=cx[clip_of], tubes=flat, targets=targets)
        loss = o[4].mean()                                       # train_cls.py:311
        return self._finish(self._backward(loss, True))

    # ---- the padded iteration: C4TrainStep's eager step, exchange, update and capture around this forward / backward
    def forward_backward(self, exchange=False):
        if self.selection == "device":                           # two launches, nothing comes back: part of the recording
            self._selected = None
            self.selection_ran = "device"
            self.selector.select(self.d_gt, self.d_gt_count, self.d_pad)
        K = self.batch * self.budget
        cf = self.base(self.x)
        cx = self.ctx(cf)
        pooled = self.nets["roi_net"](cf, self.s_flat)
        pooled = pooled.reshape(K, self.Tl, *pooled.shape[1:])
        o = self.heads[0](pooled, context_feat=self._ctx_per_tube(cx, self.budget), tubes=self.s_flat, targets=self.s_tgt)
        loss = (o[4].view(K, -1) * self.s_mask).sum() * self.s_inv[0]      # the reference's .mean() runs over the REAL rows only
        return self._backward(loss, exchange)

    def _eager_step(self):
        # (the host's selection is drawn outside a recording: capture() records this step, step() draws before each replay)
        if self.selection == "host" and not (self.x.is_cuda and torch.cuda.is_current_stream_capturing()):
            self._select_host_padded()
        return super()._eager_step()

    def step_padded(self):
        return self._eager_step()

    def capture(self, warmup=2, mode="auto"):
        """C4TrainStep.capture on the padded iteration: ONE graph ("cls-one"), or with a process group the split form ("cls-split")."""
        super().capture(warmup=warmup, mode=mode)
        self.graph_mode = "cls-" + self.graph_mode
        return self
