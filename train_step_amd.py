#!/usr/bin/env python
"""train_step_amd.py -- the one-process-per-GPU training launcher INTEGRATION.md names: what replaces the reference's
nn.DataParallel wrapping and cross-GPU head placement (train.py:142-148) around its training iteration (train.py:257-348).

    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 train_step_amd.py --iters 100
    python train_step_amd.py --iters 10                      # one GPU, no process group

Every rank
  1. joins the RCCL process group (`step_amd.dist.init`; backend "nccl" IS RCCL on ROCm, xGMI underneath),
  2. takes its slice of the global clip batch (`dist.shard_clips`: clips r, r+world, ... -- every tensor on the path is per clip and
     BN is frozen, so the shard needs no data-path collective),
  3. builds the replicas (BaseNet + ContextNet + max_iter heads; rank 0's weights are broadcast once, as DDP does at construction),
  4. captures the WHOLE step -- forward, backward with the conv weight gradients accumulated straight into FlatAdam's arena, the
     bucketed gradient all-reduce on the communication stream, the one-launch weight re-pack, the fused Adam -- in one HIP graph
     (`workloads.C4TrainStep.capture`), so the N > 1 step is the same replayed program as the N = 1 step plus its collectives,
  5. replays it --iters times, the learning-rate schedule written through `optimizer.param_groups` exactly as the reference's
     schedulers do (utils/solver.py:96-180: the captured Adam reads per-group lr / weight_decay from device tables that
     `step()` refreshes from the param groups),
     --optimizer sgd trains with the reference's default optimizer instead (train.py:123-124: SGD with momentum, step_amd.FlatSGD) --
     same arenas, same exchange, same captured step,
     --dropout P trains with the heads' dropout (the reference's recipe: 0.3) on the device-side generator: the captured step draws new masks
     on every replay (`step_amd.Dropout`, `step_amd.rng`); --rng-seed S seeds it, rank r with S + r,
     --select-device trains on the reference's whole iteration with the proposal selection on the device, drawing from the same generator: one
     graph per iteration instead of two around the host's selection; --proposals K starts it from detector proposals instead of the anchor
     grid -- a changing number per clip in K padded slots with a device-side count (`step_select_train_counted`), transformed with the
     frames under --augment-device (`step_augment_plan_tubes`),
     --cls trains the classification pre-training iteration instead (train_cls.py, the stage whose checkpoint the iteration above starts from): one
     cls_only head on boxes sampled around the ground truths, ONE graph per iteration; the host draws sampling and selection before each
     replay, --cls --select-device moves both into the graph (`step_anchor_sample`, `step_select_train`),
     --grad-wire bf16 sends the gradients as bfloat16 with error feedback (`step_amd.dist.GradWire`; --no-wire-feedback: plain rounding),
     --clip-grad-norm X clips the (exchanged) gradient to an L2 norm of X inside the step (`step_grad_norm_flat` / `step_grad_clip_flat`) and
     logs the norm; --scheduler cosine|step runs the reference's WarmupCosineLR / WarmupStepLR on the device (`step_lr_schedule`, recorded in
     the graph: the replayed iteration takes no learning rate from the host; the lr is read back on log iterations only),
  6. rank 0 prints one JSON line per --log-every iterations and a final summary (loss, ms per iteration, clips/s of the whole job).

Data: synthetic AVA-shaped clips [B,36,3,400,400] and fixed anchor tubes (there is no dataset in this repository; the reference's
loader, data/ava.py, hands over the same shapes).  --feed u8 keeps the clips as uint8 frames in pinned host memory and moves them
host -> device every iteration on a copy stream (`step_clip_from_u8` writes the captured step's input): the transfer of iteration
k + 1 runs under the replay of iteration k.  --feed u8 --augment keeps the frames at the SOURCE size (--src-size, default 256x340) and runs the
reference's training transform on the device instead (`step_amd.TubeAugmentation`: a host plan per clip over synthetic tubes, drawn in
the reference's RNG order, then one `step_clip_augment_u8` launch -- photometric distortion, crop, mirror, erase, resize to the
network's resolution -- writes the captured step's input where `step_clip_from_u8` does without the flag).  --feed u8 --augment-device
--select-device makes the decisions on the device as well (`step_amd.DeviceTubeAugmentation`: `step_augment_plan` inside the captured
iteration): the uint8 frames are the graph's input, the selection trains on the boxes that belong to the augmented pixels, and an
iteration is the frame copy and one replay.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--global-batch", type=int, default=None, help="clips of the whole job per iteration (default: 1 per rank; the reference's scripts: 8)")
    ap.add_argument("--tubes", type=int, default=5, help="tubes per clip and step")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--optimizer", default="adam", choices=["adam", "sgd"],
                    help="adam: what the reference's scripts pick (train.py:126); sgd: its default, optim.SGD with momentum (train.py:123-124)")
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd (config.py:55)")
    ap.add_argument("--weight-decay", type=float, default=None,
                    help="every group's weight decay (default: the optimizer's own -- 0 for adam, 1e-7 for sgd as config.py:57)")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="drop probability of the heads' three dropout sites (the reference's recipe: 0.3, scripts/train_step.sh:41); masks come from "
                         "the device-side generator (step_amd.Dropout), fresh on every replay of the captured step")
    ap.add_argument("--rng-seed", type=int, default=0, help="seed S of the dropout generator; rank r seeds S + r, so data-parallel ranks draw different masks")
    ap.add_argument("--warmup-iters", type=int, default=3, help="eager iterations before the capture (caches, workspaces, communicator)")
    ap.add_argument("--lr-decay-every", type=int, default=0, help="> 0: multiply every group's lr by 0.1 every that many iterations (scheduler stand-in)")
    ap.add_argument("--clip-grad-norm", type=float, default=None,
                    help="clip the gradient's L2 norm to this value in front of the optimizer launch (torch.nn.utils.clip_grad_norm_ on the device, "
                         "after the exchange); the log lines gain grad_norm")
    ap.add_argument("--scheduler", default=None, choices=["cosine", "step"],
                    help="the reference's WarmupCosineLR / WarmupStepLR (utils/solver.py:96-172) on the device, base lr = --lr, stepped once per iteration "
                         "inside the captured step (step_amd.DeviceWarmupCosineLR / DeviceWarmupStepLR)")
    ap.add_argument("--milestones", default="", help="--scheduler: comma-separated iterations (cosine: the end of each cycle; step: where the lr drops)")
    ap.add_argument("--sched-warmup-iters", type=int, default=1000,
                    help="--scheduler: iterations of linear warm-up, the schedulers' warmup_iters (--warmup-iters is the eager warm-up ahead of the capture)")
    ap.add_argument("--warmup-factor", type=float, default=0.1, help="--scheduler: the lr factor the warm-up starts from")
    ap.add_argument("--min-ratio", type=float, default=0.0, help="--scheduler cosine: the floor, as a ratio of the base lr")
    ap.add_argument("--cycle-decay", type=float, default=1.0, help="--scheduler cosine: the peak is multiplied by this after every cycle")
    ap.add_argument("--gamma", type=float, default=0.1, help="--scheduler step: the factor at every milestone")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--graph", default="auto", choices=["auto", "one", "split"])
    ap.add_argument("--select", action="store_true",
                    help="the reference's whole iteration (train.py:257-348): no-grad inference + train_select between the steps (workloads.C4SelectTrainStep, "
                         "captured as graphs around the host's selection)")
    ap.add_argument("--select-device", action="store_true",
                    help="implies --select, with the selection on the device (step_select_train, draws from the generator of --rng-seed): the whole "
                         "iteration is captured as ONE graph; the draws are not the reference's")
    ap.add_argument("--cls", action="store_true",
                    help="the classification pre-training iteration instead (train_cls.py, stage 1: workloads.C4ClsTrainStep -- one cls_only head on "
                         "boxes sampled around the ground truths, captured as ONE graph); with --select-device the sampling and the selection run on "
                         "the device (step_anchor_sample + step_select_train)")
    ap.add_argument("--grad-wire", default="fp32", choices=["fp32", "bf16"],
                    help="what the gradient exchange puts on the link: the fp32 arena, or bfloat16 with error feedback (step_amd.dist.GradWire: half the "
                         "bytes, the rounding error of what a rank sent is added to its next step's gradient)")
    ap.add_argument("--no-wire-feedback", action="store_true", help="--grad-wire bf16 without the residual arena: round, sum, widen")
    ap.add_argument("--feed", default="none", choices=["none", "u8"])
    ap.add_argument("--augment", action="store_true",
                    help="--feed u8 only: uint8 frames at --src-size, the reference's TubeAugmentation (all four switches on, scripts/train_step.sh:55-58) "
                         "applied on the device by step_clip_augment_u8")
    ap.add_argument("--augment-device", action="store_true",
                    help="--feed u8 --select-device only: the augmentation's decisions, erase noise and transformed ground truths are made on the device "
                         "too (step_augment_plan, draws from the generator of --rng-seed, not numpy's), inside the captured iteration")
    ap.add_argument("--proposals", type=int, default=0, metavar="K",
                    help="--select-device only: the initial tubes are detector proposals, a changing number per clip in K padded slots with a "
                         "device-side count (synthetic here; a clip without any falls back to the anchors), instead of the anchor grid; with "
                         "--augment-device the planner transforms them with the frames")
    ap.add_argument("--temporal-mode", default="predict", choices=["predict", "extrapolate", "mean"],
                    help="--select / --select-device: how the tubes grow from one chunk to three (config.py:92 --temporal_mode): the head's neighbour "
                         "regressions, linear extrapolation of the tube's own boxes, or its mean box (step_tube_update_mode, step_tube_grow)")
    ap.add_argument("--src-size", default="256x340", help="--augment / --augment-device: HxW of the decoded source frames")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--backend", default=None, choices=["nccl", "gloo"],
                    help="process-group backend (default: nccl = RCCL; gloo only to exercise the multi-rank program with ranks SHARING one GPU, "
                         "which RCCL refuses -- the exchange is then one eager flat all-reduce between two captured graphs)")
    a = ap.parse_args()
    if a.cls and (a.feed != "none" or a.graph == "one" or a.select or a.tubes != ap.get_default("tubes")):
        raise SystemExit("train_step_amd.py: --cls takes none of --feed, --graph one, --select and --tubes (its tubes are sampled around the "
                         "ground truths; --select-device moves that sampling and the selection onto the device)")
    a.select = (a.select or a.select_device) and not a.cls
    if a.optimizer == "sgd" and a.momentum <= 0:
        raise SystemExit("train_step_amd.py: --momentum must be positive (the workload's momentum buffer is allocated at construction)")
    if a.augment and a.feed != "u8":
        raise SystemExit("train_step_amd.py: --augment needs --feed u8 (the augmentation reads the uint8 frames)")
    if a.augment_device and (a.feed != "u8" or not a.select_device or a.cls or a.augment):
        raise SystemExit("train_step_amd.py: --augment-device needs --feed u8 --select-device (the device selection reads the boxes the planner "
                         "writes), without --cls and --augment")
    if a.proposals and (a.proposals < 0 or not a.select_device or a.cls):
        raise SystemExit("train_step_amd.py: --proposals K needs --select-device (the host selection keeps its ragged form), without --cls, and K >= 1")
    if a.temporal_mode != "predict" and not a.select:
        raise SystemExit("train_step_amd.py: --temporal-mode needs --select or --select-device (only the selecting iteration grows tubes from predictions)")
    if a.scheduler and a.lr_decay_every:
        raise SystemExit("train_step_amd.py: --scheduler and --lr-decay-every both write the learning rate; pick one")
    if a.clip_grad_norm is not None and not a.clip_grad_norm > 0:
        raise SystemExit("train_step_amd.py: --clip-grad-norm must be positive")
    if not torch.cuda.is_available():
        raise SystemExit("train_step_amd.py needs a ROCm device (there is no CPU fallback)")

    import step_amd
    from step_amd import dist as sdist, ops, workloads
    rank, world = sdist.init(a.backend)
    local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    gb = a.global_batch or world
    mine = sdist.shard_clips(gb, rank, world)
    if len(set(len(sdist.shard_clips(gb, r, world)) for r in range(world))) != 1:
        raise SystemExit("train_step_amd.py: --global-batch must be a multiple of the world size (equal shards keep the mean-of-means "
                         "equal to the single-process loss, SURVEY 8e)")
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    graphed = not a.no_graph and a.dtype != "f32"               # (the fp32 step is GPU-bound and measured slower replayed than eager)
    lr_schedule = None
    if a.scheduler:
        milestones = [int(v) for v in a.milestones.split(",") if v.strip()]

        def lr_schedule(opt):
            for g in opt.param_groups:                            # the schedule's base lr is --lr (the workload builds its optimizer with its own)
                g["lr"] = a.lr
            if a.scheduler == "cosine":
                return step_amd.DeviceWarmupCosineLR(opt, milestones, min_ratio=a.min_ratio, cycle_decay=a.cycle_decay, warmup_iters=a.sched_warmup_iters,
                                                     warmup_factor=a.warmup_factor)
            return step_amd.DeviceWarmupStepLR(opt, milestones, gamma=a.gamma, warmup_iters=a.sched_warmup_iters, warmup_factor=a.warmup_factor)
    extra = dict(max_grad_norm=a.clip_grad_norm, lr_schedule=lr_schedule)
    capturable = graphed or bool(a.scheduler)                    # (a device scheduler wants the device-counted optimizer, captured or not)
    if a.cls:
        import random
        import numpy as np
        random.seed(1000 + rank)                                 # (the host's sampling and selection draw from the reference's two RNG streams)
        np.random.seed(1000 + rank)
        w = workloads.C4ClsTrainStep(dev, batch=len(mine), seed=123 + rank, dtype=tdt, capturable=capturable, optimizer=a.optimizer, dropout=a.dropout,
                                     rng_seed=a.rng_seed + rank, selection="device" if a.select_device else "host", grad_wire=a.grad_wire,
                                     wire_feedback=not a.no_wire_feedback, **extra)
    elif a.select:
        import random
        import numpy as np
        random.seed(1000 + rank)                                 # (the selection draws from the reference's two host RNG streams)
        np.random.seed(1000 + rank)
        if a.augment_device:                                     # (400 x 400: the workload's clips; the generator is the workload's)
            extra.update(augment=step_amd.DeviceTubeAugmentation((400, 400), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2),
                         src_size=tuple(int(v) for v in a.src_size.lower().split("x")))
        if a.proposals:
            extra.update(proposals=a.proposals)
        w = workloads.C4SelectTrainStep(dev, batch=len(mine), seed=123 + rank, dtype=tdt, capturable=capturable, optimizer=a.optimizer,
                                        dropout=a.dropout, rng_seed=a.rng_seed + rank, selection="device" if a.select_device else "host",
                                        grad_wire=a.grad_wire, wire_feedback=not a.no_wire_feedback, temporal_mode=a.temporal_mode, **extra)
    else:
        w = workloads.C4TrainStep(dev, batch=len(mine), tubes_per_clip=a.tubes, seed=123 + rank, dtype=tdt, capturable=capturable,
                                  optimizer=a.optimizer, dropout=a.dropout, rng_seed=a.rng_seed + rank, grad_wire=a.grad_wire,
                                  wire_feedback=not a.no_wire_feedback, **extra)
    for g in w.opt.param_groups:
        g["lr"] = a.lr
        if a.optimizer == "sgd":
            g["momentum"] = a.momentum
        if a.weight_decay is not None:
            g["weight_decay"] = a.weight_decay
    # --select-device without a capture (--no-graph, fp32): the padded eager iteration, which selects on the device -- the ragged step() always
    # selects on the host
    run = w.step_padded if (a.select_device and not graphed) else w.step
    if graphed:
        w.capture(warmup=a.warmup_iters, mode=a.graph)             # (C4SelectTrainStep: its own graph forms; `mode` only matters for the fixed-tube step)
    else:
        for _ in range(a.warmup_iters):
            run()

    feed = None
    if a.augment_device:
        # the uint8 frames are the captured iteration's input.  Host -> device on a copy stream into one of two landing buffers, under the
        # replay of the iteration before (the prefetch of --feed u8 below); then ONE device copy into the workload's stage buffer and the
        # replay, which plans, augments, selects and trains without the host
        g_ = torch.Generator().manual_seed(999 + rank)
        host = [torch.randint(0, 256, tuple(w.stage.shape), dtype=torch.uint8, generator=g_).pin_memory() for _ in range(2)]
        landed = [torch.empty_like(w.stage) for _ in range(2)]
        copy_stream = torch.cuda.Stream()
        copied = [torch.cuda.Event() for _ in range(2)]
        main_stream = torch.cuda.current_stream()

        def prefetch(k):
            with torch.cuda.stream(copy_stream):
                landed[k % 2].copy_(host[k % 2], non_blocking=True)
                copied[k % 2].record(copy_stream)

        def feed(k):
            main_stream.wait_event(copied[k % 2])
            w.stage.copy_(landed[k % 2])
            copy_stream.wait_stream(main_stream)
            prefetch(k + 1)
        prefetch(0)
    elif a.feed == "u8":
        N, T, _, H, W = w.x.shape
        g_ = torch.Generator().manual_seed(999 + rank)
        Hs, Ws = (int(v) for v in a.src_size.lower().split("x")) if a.augment else (H, W)
        host = [torch.randint(0, 256, (N, T, Hs, Ws, 3), dtype=torch.uint8, generator=g_).pin_memory() for _ in range(2)]
        stage = [torch.empty((N, T, Hs, Ws, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        if a.augment:
            import numpy as np
            from step_amd import TubeAugmentation
            np.random.seed(2000 + rank)                           # (the plans draw from numpy's global stream, as the reference's transform does)
            aug = TubeAugmentation((W, H), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2)
            centre = np.random.uniform(0.35, 0.65, (N, 2, 1, 2))
            half = np.random.uniform(0.1, 0.25, (N, 2, 1, 2))
            gt_tubes = np.tile(np.concatenate([centre - half, centre + half], 3), (1, 1, T, 1)).astype(np.float32)   # two synthetic tubes per clip
        # a stream of its own at DEFAULT priority.  (Round 5 gave it high priority, as bench.py's forward-only fed loop does; beside the captured
        # TRAINING step -- whose graph forks onto side streams -- a high-priority stream that spends its time waiting on the main stream made
        # the whole iteration 3x slower: 40.3 against 13.6 ms, tools/feed_train_probe.py, profiles/r06_feed_train_probe.txt)
        copy_stream = torch.cuda.Stream()
        copied = [torch.cuda.Event() for _ in range(2)]
        main_stream = torch.cuda.current_stream()

        def prefetch(k):
            with torch.cuda.stream(copy_stream):
                stage[k % 2].copy_(host[k % 2], non_blocking=True)
                copied[k % 2].record(copy_stream)

        def feed(k):
            main_stream.wait_event(copied[k % 2])
            if a.augment:                                        # what a dataset worker does per clip (host, no pixels) + one launch for the batch
                plans = [aug.plan((T, Hs, Ws), gt_tubes[n])[0] for n in range(N)]
                aug.apply(stage[k % 2], plans, out=w.x)
            else:
                ops.clip_from_u8(stage[k % 2], scale=2, out=w.x)     # the captured step's static input
            copy_stream.wait_stream(main_stream)                 # (the next copy into the OTHER buffer may start at once; this one is re-used at k + 2)
            prefetch(k + 1)
        prefetch(0)

    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    tl = t0
    for it in range(a.iters):
        if a.lr_decay_every and it and it % a.lr_decay_every == 0:
            for g in w.opt.param_groups:                          # what utils/solver.py's schedulers do between iterations
                g["lr"] *= 0.1
        if feed is not None:
            feed(it)
        loss = run()
        if rank == 0 and a.log_every and (it + 1) % a.log_every == 0:
            lv = float(loss)                                      # (one host sync per log line)
            now = time.perf_counter()
            lr = w.sched.get_last_lr()[0] if w.sched is not None else w.opt.param_groups[0]["lr"]     # (device schedule: read back here only)
            norm = {"grad_norm": round(float(w.opt.grad_norm[0]), 6)} if a.clip_grad_norm is not None else {}
            print(json.dumps({"iter": it + 1, "loss": round(lv, 6), "ms_per_iter": round((now - tl) / a.log_every * 1e3, 3), "lr": lr, **norm}),
                  flush=True)
            tl = now
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=dev if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        el = float(t.item())
    # every rank prints the float64 sum of its parameter arena: replicas that apply the same exchanged gradient hold the same number
    checksum = float(w.opt.flat_param.double().sum().item())
    if rank != 0:
        print(json.dumps({"rank": rank, "param_checksum": checksum}), flush=True)
    if rank == 0:
        print(json.dumps({"summary": True, "world_size": world, "global_batch": gb, "clips_per_rank": len(mine), "iters": a.iters,
                          "ms_per_iter": round(el / max(a.iters, 1) * 1e3, 3), "clips_per_s": round(gb * a.iters / el, 3),
                          "launch": ("hipGraph replay (%s)" % w.graph_mode) if w.graph is not None else "eager",
                          "gradient_exchange": _exchange_label(w, world),
                          "grad_wire": a.grad_wire, "exchange_bytes_per_step": w.opt.numel * (2 if a.grad_wire == "bf16" else 4), "param_checksum": checksum,
                          "feed": a.feed + ("+augment" if a.augment else "+augment-device" if a.augment_device else ""),
                          **({"gt_kept": int(w.d_gt_count.sum().item())} if a.augment_device else {}),
                          **({"proposals": a.proposals, "proposals_real": int(w.d_count.sum().item())} if a.proposals else {}), "dtype": a.dtype, "final_loss": round(float(w.loss), 6), "optimizer": a.optimizer, "opt_steps": w.opt.step_count,
                          "dropout": a.dropout, "rng_offset": w.rng.offset(), **({"selection": w.selection_ran} if (a.select or a.cls) else {}),
                          **({"temporal_mode": a.temporal_mode} if a.select else {}),
                          **({"workload": "cls"} if a.cls else {}),
                          **({"clip_grad_norm": a.clip_grad_norm, "grad_norm": round(float(w.opt.grad_norm[0]), 6)} if a.clip_grad_norm is not None else {}),
                          **({"scheduler": a.scheduler, "last_epoch": w.sched.last_epoch, "lr": w.sched.get_last_lr()[0]} if w.sched is not None else {}),
                          **({"adam_steps": w.opt.step_count} if a.optimizer == "adam" else {})}), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def _exchange_label(w, world):
    """What the step's gradient exchange really was: the split form and gloo run ONE eager flat all-reduce, not the buckets."""
    if not w.reducer.active:
        return None
    backend = torch.distributed.get_backend()
    lib = "RCCL" if backend == "nccl" else backend
    if getattr(w, "graph_mode", None) in ("split", "select-split", "select-one-split", "cls-split"):
        return "one eager flat %s all-reduce of the gradient arena between the two graphs, %d ranks" % (lib, world)
    where = "recorded in the step's graph" if w.graph is not None else "eager, overlapped with backward"
    return "bucketed %s all-reduce, %d buckets, %s, %d ranks" % (lib, len(w.reducer.buckets), where, world)


if __name__ == "__main__":
    main()
