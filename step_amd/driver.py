"""step_amd/driver.py -- the multi-step inference driver over the HIP modules.

Counterpart of utils/utils.py:15-131 (`inference`): per step, ROI-pool the current tubes out of the
backbone feature, run that step's TwoBranchNet, decode the regressed boxes, and (between steps 2 and
3 of the default schedule) extend the tubes in time with the predicted neighbours.  Same `history`
contract: a list with one dict per step holding pred_prob [N,Tl,classes], pred_loc [N,Tl,4],
pred_first_loc / pred_last_loc [N,T,4] and tubes_nums.

Differences from the reference's host glue (they do not change results):
  * everything stays on the device between steps: the tube bookkeeping is tensor ops, there is no
    per-tube `.item()` (utils.py:57), no numpy round trip (utils.py:107-125), no per-box Python loop
    (tube_utils.py:84-88);
  * the ROI-pooled features are produced channels-last by the NHWC ROIAlign kernel straight from the
    channels-last backbone feature (no `.contiguous()` transpose of the slice, utils.py:48).
All three temporal modes of the reference are implemented (utils.py:102-120): "predict" (every shipped script: the head's
neighbour regressions extend the tube), "extrapolate" (linear, tube_utils.py:159-176; config.py:92's default) and "mean".  In all three
a step's bookkeeping is ONE launch (step_tube_update; step_tube_update_mode for the other two, which grow a tube from its own boxes);
TUBE_KERNEL = False keeps the tensor-op restatement of each.
"""
import numpy as np
import torch

from . import ops
from .tube_math import extrapolate_tubes, decode_coef, valid_tubes

TUBE_KERNEL = True             # per-step tube bookkeeping as one HIP launch, in every temporal mode (False: the tensor-op restatement below)
COMPACT_KERNEL = True          # postprocess: the detection rows of all iterations and clips compacted by one HIP launch (False: nonzero / gather / bincount);
                               # postprocess_merged always compacts with the launch: step_detect_merge reads its segments
DETECT_BLOCK = True            # clips of 65 .. 1024 tubes take the fused path too (step_detect_nms' workgroup form); False: they go through
                               # _general_rows (tensor operations around step_nms_batched), the routing before that form existed
DETECT_TUBES_MAX = 1024        # STEP_DETECT_TUBES_MAX
MERGE_ROWS_MAX = 65536         # step_detect_merge's bitmap: rows per (iteration, clip) segment


def _fused_tubes():
    """the most tubes per clip that the fused evaluation path takes"""
    return DETECT_TUBES_MAX if DETECT_BLOCK else 64


def _flat_tubes(tubes_list, device, dtype=torch.float32):
    """list (one per clip) of [n_i, T, 4] tensors/arrays -> flat [sum n_i, T, 5] with frame index, nums"""
    rows, nums = [], []
    for b, t in enumerate(tubes_list):
        t = torch.as_tensor(t, dtype=dtype, device=device)
        nums.append(int(t.shape[0]))
        if t.shape[0] == 0:
            continue
        T = t.shape[1]
        idx = (torch.arange(T, device=device, dtype=dtype) + b * T).view(1, T, 1).expand(t.shape[0], T, 1)
        rows.append(torch.cat([idx, t], dim=2))
    return torch.cat(rows, dim=0), nums


def pad_tubes(tubes_list, capacity, device, width, height):
    """list (one per clip) of [n_i, T, 4] tensors/arrays, n_i <= capacity (zero included) -> (flat [B*K,T,5] with the frame index, count
    int32 [B]), K = capacity: the padded form of _flat_tubes.  A clip owns K slots, the first count[b] hold its tubes, the others the whole
    frame (0, 0, width, height) on every frame -- a valid box for ROIAlign, what valid_tubes makes of a degenerate one.  inference_flat(...,
    counts=count) carries the count to postprocess, which hands it to step_detect_nms."""
    K, B = int(capacity), len(tubes_list)
    arrs = [np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, np.float32) for t in tubes_list]
    T = next((a.shape[1] for a in arrs if a.ndim == 3), None)
    if T is None:
        raise ValueError("step_amd: pad_tubes wants [n,T,4] arrays (an empty clip is a [0,T,4] array)")
    arrs = [a.reshape(-1, T, 4) for a in arrs]
    host = np.empty((B, K, T, 5), np.float32)
    host[..., 1:] = (0.0, 0.0, float(width), float(height))
    host[..., 0] = (np.arange(B, dtype=np.float32)[:, None, None] * T + np.arange(T, dtype=np.float32)[None, None, :])
    count = np.zeros(B, np.int32)
    for b, a in enumerate(arrs):
        if a.shape[0] > K:
            raise ValueError("step_amd: clip %d has %d tubes, the capacity is %d" % (b, a.shape[0], K))
        host[b, :a.shape[0], :, 1:] = a
        count[b] = a.shape[0]
    return torch.from_numpy(host.reshape(B * K, T, 5)).to(device), torch.from_numpy(count).to(device)


def inference(args, conv_feat, context_feat, nets, exec_iter, tubes):
    """args: Namespace with T, NUM_CHUNKS, max_iter, num_classes, image_size, no_context, temporal_mode
    conv_feat [B,T_all,C,H,W] (BaseNet output), context_feat [B,1024,T_all,1,1] or None,
    nets: {'roi_net': ROINet, 'det_net0': TwoBranchNet, ...}, tubes: list of [n_i,T,4] per clip.
    Returns (history, trajectory) in the reference's form: history[i] = {pred_prob [N,Tl,classes], pred_loc [N,Tl,4],
    pred_first_loc / pred_last_loc [N,T,4] (None unless temporal_mode == "predict"), tubes_nums}, detached;
    trajectory[i] = per clip (numpy proposals for the next step, class index [n,Tl])."""
    if getattr(args, "temporal_mode", "predict") not in ("predict", "extrapolate", "mean"):
        raise NotImplementedError("step_amd.driver.inference: temporal_mode %r" % (args.temporal_mode,))
    dev = conv_feat.device
    flat, nums = _flat_tubes(tubes, dev)
    clip_of = torch.as_tensor(np.repeat(np.arange(len(nums)), nums), device=dev)
    history, traj = inference_flat(args, conv_feat, context_feat, nets, exec_iter, flat, nums, clip_of)
    # the reference's trajectory (utils.py:87-124): per step, per clip (numpy proposals [n,T',4], class index [n,Tl])
    trajectory = []
    for (prop, cls), h in zip(traj, history):
        Tl = h["pred_loc"].shape[1]
        props = np.split(prop.detach().cpu().numpy(), np.cumsum(nums)[:-1], axis=0)
        classes = torch.split(cls.view(-1, 1).expand(-1, Tl), nums, dim=0)
        trajectory.append(list(zip(props, classes)))
    return history, trajectory


def inference_flat(args, conv_feat, context_feat, nets, exec_iter, flat, nums, clip_of, want_classes=True, counts=None):
    """The device-resident core of `inference`: flat [N,T,5] tubes (col 0 = frame index), nums = tubes per
    clip, clip_of [N] = clip index of every tube.  Pure tensor ops with static shapes and no host
    synchronisation, so the whole multi-step pipeline can be captured in a hipGraph (GraphedInference).
    want_classes=False: the trajectory's class index (an argmax per step that only `inference` hands on) is None.
    counts: int32 [B] on the device for PADDED clips (pad_tubes: nums = [K] * B slots, the first counts[b] of a clip real) -- every
    history dict then carries it as "tubes_count" beside "tubes_nums"; the arithmetic runs over all slots."""
    dev = conv_feat.device
    history, trajectory = [], []
    clip32 = None
    for i in range(1, exec_iter + 1):
        chunks = args.NUM_CHUNKS[i]
        T_start = int((args.NUM_CHUNKS[args.max_iter] - chunks) / 2) * args.T
        T_length = chunks * args.T
        chunk_idx = [j * args.T + int(args.T / 2) for j in range(chunks)]
        half_T = int(args.T / 2)

        pooled = nets["roi_net"](conv_feat[:, T_start:T_start + T_length], flat)       # [N*Tl, C, 7, 7]
        pooled = pooled.reshape(-1, T_length, *pooled.shape[1:])
        ctx = None
        if not args.no_context:
            ctx = context_feat[clip_of][:, :, T_start:T_start + T_length]               # utils.py:55-57, batched
        prob, local_loc, first_loc, last_loc, _, _, _ = nets["det_net%d" % (i - 1)](pooled, context_feat=ctx)

        pred_prob = prob.view(-1, 1, args.num_classes).expand(-1, T_length, -1)
        mode = getattr(args, "temporal_mode", "predict")
        extend = i < args.max_iter and args.NUM_CHUNKS[i + 1] == args.NUM_CHUNKS[i] + 2
        if mode == "predict" and TUBE_KERNEL and first_loc is not None and last_loc is not None and flat.shape[1] == T_length:
            # decode x3 -> cat -> valid_tubes -> frame-index column: one launch (step_tube_update) instead of ~60 element-wise ones
            if clip32 is None:
                clip32 = clip_of.to(torch.int32)
            pred_loc, pred_first, pred_last, flat = ops.tube_update(
                flat, local_loc, first_loc, last_loc, clip32, chunk_idx[0] - half_T, chunk_idx[-1] - half_T, extend,
                args.image_size[0], args.image_size[1])
            history.append({"pred_prob": pred_prob.detach(), "pred_loc": pred_loc, "pred_first_loc": pred_first,
                            "pred_last_loc": pred_last, "tubes_nums": list(nums)})
            if counts is not None:
                history[-1]["tubes_count"] = counts
            trajectory.append((flat[:, :, 1:], torch.argmax(prob, dim=-1) if want_classes else None))
            continue
        if mode in ("extrapolate", "mean") and TUBE_KERNEL and local_loc is not None and flat.shape[1] == T_length:
            # decode -> extrapolate_tubes / mean tiling -> valid_tubes -> frame-index column: one launch (step_tube_update_mode); the head's
            # neighbour regressions are neither decoded nor kept in these modes (utils.py:83-84)
            if clip32 is None:
                clip32 = clip_of.to(torch.int32)
            pred_loc, flat = ops.tube_update_mode(flat, local_loc, clip32, mode, extend, args.T, args.image_size[0], args.image_size[1])
            history.append({"pred_prob": pred_prob.detach(), "pred_loc": pred_loc, "pred_first_loc": None, "pred_last_loc": None,
                            "tubes_nums": list(nums)})
            if counts is not None:
                history[-1]["tubes_count"] = counts
            trajectory.append((flat[:, :, 1:], torch.argmax(prob, dim=-1) if want_classes else None))
            continue
        flat = flat.to(local_loc)
        pred_loc = decode_coef(flat.reshape(-1, 5)[:, 1:], local_loc.reshape(-1, 4)).view(local_loc.shape)
        lo, hi = chunk_idx[0] - half_T, chunk_idx[0] + half_T + 1
        lo2, hi2 = chunk_idx[-1] - half_T, chunk_idx[-1] + half_T + 1
        pred_first = decode_coef(flat[:, lo:hi].reshape(-1, 5)[:, 1:], first_loc.reshape(-1, 4)).view(first_loc.shape)
        pred_last = decode_coef(flat[:, lo2:hi2].reshape(-1, 5)[:, 1:], last_loc.reshape(-1, 4)).view(last_loc.shape)
        history.append({"pred_prob": pred_prob.detach(), "pred_loc": pred_loc.detach(),            # utils.py:81-85 (.data)
                        "pred_first_loc": pred_first.detach() if mode == "predict" else None,
                        "pred_last_loc": pred_last.detach() if mode == "predict" else None, "tubes_nums": list(nums)})
        if counts is not None:
            history[-1]["tubes_count"] = counts

        # next step's proposals (utils.py:91-129), all clips at once
        if extend:
            if mode == "predict":
                prop = torch.cat([pred_first, pred_loc, pred_last], dim=1)
            elif mode == "extrapolate":
                prop = extrapolate_tubes(pred_loc, args.T)
            else:                                               # the tube's mean box on both sides (utils.py:116-120)
                # np.mean's arithmetic, bit for bit: the sequential fp32 sum in frame order, DIVIDED by the frame count.  torch's mean, and
                # its division by a host scalar, multiply by fl(1 / Tl) instead (a third of the values differ in the last bit at Tl = 3):
                # the divisor is a device tensor
                s = pred_loc[:, 0]
                for t in range(1, pred_loc.shape[1]):
                    s = s + pred_loc[:, t]
                m = (s / torch.full_like(s, float(pred_loc.shape[1]))).unsqueeze(1).expand(-1, args.T, -1)
                prop = torch.cat([m, pred_loc, m], dim=1)
        else:
            prop = pred_loc
        prop = valid_tubes(prop, width=args.image_size[0], height=args.image_size[1])
        trajectory.append((prop, torch.argmax(prob, dim=-1) if want_classes else None))
        Tn = prop.shape[1]
        idx = (clip_of.to(prop.dtype) * Tn).view(-1, 1, 1) + torch.arange(Tn, device=dev, dtype=prop.dtype).view(1, Tn, 1)
        flat = torch.cat([idx, prop], dim=2)
    return history, trajectory


def _clip_groups(nums, device):
    """Index tables of the ragged (clip, tube) layout: gather index [B,kmax] into the flat tube axis (clamped) and the
    validity mask [B,kmax]; built from host ints without touching the device data."""
    B, kmax = len(nums), max(max(nums), 1)
    n = torch.as_tensor(nums, device=device, dtype=torch.int64)
    start = torch.cumsum(n, 0) - n
    j = torch.arange(kmax, device=device, dtype=torch.int64)
    valid = j.view(1, kmax) < n.view(B, 1)
    idx = (start.view(B, 1) + j.view(1, kmax)).clamp_(max=max(int(sum(nums)) - 1, 0))
    return idx, valid


_POST_CONST = {}


def _count32(count, B, dev):
    if tuple(count.shape) != (B,) or count.device != dev:
        raise RuntimeError("step_amd: a history's tubes_count wants an int32 [B=%d] tensor on %s, got %s on %s" % (B, dev, tuple(count.shape), count.device))
    return count if count.dtype == torch.int32 and count.is_contiguous() else count.to(torch.int32).contiguous()


def _count_key(h):
    """histories that share a clip layout share a launch: a padded one's count tensor is part of its layout"""
    c = h.get("tubes_count")
    return None if c is None else (c.data_ptr(), c._version)


def _detect_keep(nums, NC, dev, members, conf, thr, W, H, count=None):
    """The fused mask + valid_tubes + NMS launch (ops.detect_nms) of every iteration in `members` (one clip layout `nums`, <= 1024 tubes
    per clip: a wavefront per (clip, class) up to 64, a workgroup beyond) -> keep [I,B,NC,kmax], the clamped boxes and the middle-frame
    scores per iteration, tube_start [B] int32, [W,H,W,H].  count: a padded history's "tubes_count" -- `nums` are then the clips' SLOTS and the
    launch takes its tube_count from that device tensor instead of the cached table: padded slots are never kept."""
    B, kmax, I = len(nums), max(nums), len(members)
    # per-layout constants live on the device (a host -> device copy from pageable memory per call stalls the host; the layout of a
    # serving loop never changes)
    ck = (nums, dev, W, H)
    hit = _POST_CONST.get(ck)
    if hit is None:
        n = torch.as_tensor(nums, device=dev, dtype=torch.int32)
        hit = _POST_CONST[ck] = (n, (torch.cumsum(n, 0) - n).to(torch.int32), torch.tensor([W, H, W, H], device=dev))
        if len(_POST_CONST) > 64:
            _POST_CONST.pop(next(iter(_POST_CONST)))
    n, start, whwh = hit
    if count is not None:
        n = _count32(count, B, dev)
    keep = torch.empty((I, B, NC, kmax), dtype=torch.uint8, device=dev)
    sc_all, bx_all = [], []
    for k, (oi, h) in enumerate(members):
        prob, loc = h["pred_prob"], h["pred_loc"]
        scores = prob[:, int(prob.shape[1] / 2)].float()                                          # [N,NC] middle frame (test.py:159)
        _, boxes = ops.detect_nms(scores, loc[:, int(loc.shape[1] / 2)].float(), start, n, kmax, conf, thr, 400.0, 400.0, keep[k])
        sc_all.append(scores)                                                                     # (valid_tubes' 400 x 400 default, as the reference calls it: test.py:161,191)
        bx_all.append(boxes)
    return keep, bx_all, sc_all, start, whwh


def postprocess(args, history, conf_thresh=None, nms_thresh=None, evaluate_topk=None, topk=None, iterations=None):
    """The evaluation loop of test.py:157-210 (the same code is inlined in train.py:512-573 and demo.py:123-174) as batched
    tensor operations: for EVERY refinement iteration and every clip, per class: mask the middle-frame scores with
    `score > conf_thresh`, valid_tubes() the middle-frame boxes (its 400 x 400 default, as the reference calls it), greedy
    NMS, normalise by the frame size; then the reference's row order -- classes ascending, kept tubes in ascending original
    order -- or, with evaluate_topk > 0, its stable ascending score sort, reversed, cut at `[:args.topk]` (including what that
    slice does for topk = -1).  The score mask, valid_tubes and the NMS of all (clip, class) groups of an iteration are ONE launch
    (step_detect_nms; the reference makes 60 x B serial CPU calls), there is no Python loop over classes or boxes, and ONE host
    synchronisation for all iterations fetches the row counts for the per-clip split.

    Thresholds default to args.conf_thresh / nms_thresh / evaluate_topk / topk (config.py:62-65).
    Returns a list over iterations of lists over clips of dicts {boxes [m,4] fp32 normalised, scores [m], labels [m] (class
    index), tubes [m] (index of the tube inside its clip)} in the order the reference writes its CSV rows."""
    conf = float(getattr(args, "conf_thresh", 0.01) if conf_thresh is None else conf_thresh)
    thr = float(getattr(args, "nms_thresh", 0.4) if nms_thresh is None else nms_thresh)
    etopk = int(getattr(args, "evaluate_topk", -1) if evaluate_topk is None else evaluate_topk)
    topk = int(getattr(args, "topk", -1) if topk is None else topk)
    W, H = float(args.image_size[0]), float(args.image_size[1])
    todo = [(it, h) for it, h in enumerate(history) if iterations is None or it in iterations]
    out = [None] * len(todo)
    # iterations that share a clip layout (they all do in inference()) go through ONE pass: a fused mask + clamp + NMS launch each
    # (ops.detect_nms), then one nonzero over all of them and ONE host synchronisation for the row counts
    fast, slow = [], []
    for oi, (it, h) in enumerate(todo):
        nums = [int(v) for v in h["tubes_nums"]]
        if len(nums) == 0 or sum(nums) == 0:
            e = torch.zeros(0, device=h["pred_loc"].device)
            out[oi] = [{"boxes": e.view(0, 4), "scores": e, "labels": e.long(), "tubes": e.long()} for _ in nums]
        elif max(nums) <= _fused_tubes():
            fast.append((oi, h, nums))
        elif h.get("tubes_count") is not None:
            raise NotImplementedError("step_amd: a padded history (tubes_count) takes the fused path: at most %d slots per clip" % _fused_tubes())
        else:
            slow.append((oi, h, nums))
    groups = {}
    for oi, h, nums in fast:
        groups.setdefault((tuple(nums), h["pred_prob"].shape[-1], h["pred_loc"].device, _count_key(h)), []).append((oi, h))
    for (nums, NC, dev, _), members in groups.items():
        B, kmax, I = len(nums), max(nums), len(members)
        keep, bx_all, sc_all, start, whwh = _detect_keep(nums, NC, dev, members, conf, thr, W, H, members[0][1].get("tubes_count"))
        # rows in the reference's order: iteration, clip, class ascending, kept tube ascending == row-major order of `keep`
        if COMPACT_KERNEL and I <= 8:
            # one launch (step_detect_compact: a ballot prefix per (iteration, clip) into fixed-capacity segments) and one small copy of
            # the row counts -- before: nonzero + index + cat + gather + bincount, ~25 launches (~100 us of the GPU per step at 4 x 34
            # tubes) and two host synchronisations
            rb_, rs_, kc_, kj_, cnt = ops.detect_compact(keep, bx_all, sc_all, start, W, H)
            per = cnt.tolist()                                                                        # the one host sync
            cap = NC * kmax
            pieces = [(rb_[g * cap:g * cap + per[g]], rs_[g * cap:g * cap + per[g]], kc_[g * cap:g * cap + per[g]], kj_[g * cap:g * cap + per[g]])
                      for g in range(I * B)]
        else:
            ki, kb, kc, kj = torch.nonzero(keep, as_tuple=True)
            tube = start.long()[kb] + kj + ki * sum(nums)
            rb = torch.cat(bx_all)[tube] / whwh                                                       # test.py:197-198
            rs = torch.cat(sc_all)[tube, kc]
            per = torch.bincount(ki * B + kb, minlength=I * B).tolist()                               # the one host sync
            pieces = list(zip(rb.split(per), rs.split(per), kc.split(per), kj.split(per)))
        for k, (oi, h) in enumerate(members):
            clips = []
            for bx, sc, cl, tb in pieces[k * B:(k + 1) * B]:
                if etopk > 0:                                                                         # test.py:205-208
                    # list.sort(key=score) is stable and ascending, then reversed: descending with ties in REVERSED row order
                    sel = torch.flip(torch.argsort(sc, stable=True), dims=(0,))[:topk]
                    bx, sc, cl, tb = bx[sel], sc[sel], cl[sel], tb[sel]
                clips.append({"boxes": bx, "scores": sc, "labels": cl, "tubes": tb})
            out[oi] = clips
    for oi, h, nums in slow:
        out[oi] = _postprocess_general(h, nums, conf, thr, etopk, topk, W, H)
    return out


def _general_rows(h, nums, conf, thr, W, H):
    """The rows of one iteration on the general path, all clips in one flat list in the reference's order: (clip, class, box, score,
    tube) per row."""
    from .roi_layers import nms_batched
    prob, loc = h["pred_prob"], h["pred_loc"]
    dev = loc.device
    B, NC = len(nums), prob.shape[-1]
    boxes = valid_tubes(loc[:, int(loc.shape[1] / 2)].float().unsqueeze(1))[:, 0]                     # [N,4] (test.py:161,191)
    scores = prob[:, int(prob.shape[1] / 2)].float()                                                  # [N,NC] (:159)
    idx, valid = _clip_groups(nums, dev)
    kmax = idx.shape[1]
    gs = scores[idx].permute(0, 2, 1)                                                                 # [B,NC,kmax]
    mask = (gs > conf) & valid.view(B, 1, kmax)                                                       # :180
    # the reference compacts the masked boxes before nms (order kept): move them to the front of each group
    order = torch.argsort((~mask).to(torch.int8), dim=2, stable=True)
    gs = torch.gather(gs, 2, order)
    gb = boxes[idx].view(B, 1, kmax, 4).expand(B, NC, kmax, 4)
    gb = torch.gather(gb, 2, order.unsqueeze(-1).expand(B, NC, kmax, 4)).contiguous()
    counts = mask.sum(2).to(torch.int32)
    keep = nms_batched(gb.view(B * NC, kmax, 4), gs.reshape(B * NC, kmax), counts.view(-1), thr).view(B, NC, kmax).bool()
    kb, kc, kj = torch.nonzero(keep, as_tuple=True)
    rb = gb[kb, kc, kj] / torch.tensor([W, H, W, H], device=dev)                                      # :197-198
    rs = gs[kb, kc, kj]
    rt = order[kb, kc, kj]
    return kb, kc, rb, rs, rt


def _postprocess_general(h, nums, conf, thr, etopk, topk, W, H):
    """One iteration with tensor operations + step_nms_batched: more than 1024 tubes per clip (more than 64 with DETECT_BLOCK = False), and
    the exact comparison for the fused path."""
    B = len(nums)
    kb, kc, rb, rs, rt = _general_rows(h, nums, conf, thr, W, H)
    per_clip = torch.bincount(kb, minlength=B).tolist()
    clips = []
    for bx, sc, cl, tb in zip(rb.split(per_clip), rs.split(per_clip), kc.split(per_clip), rt.split(per_clip)):
        if etopk > 0:
            sel = torch.flip(torch.argsort(sc, stable=True), dims=(0,))[:topk]
            bx, sc, cl, tb = bx[sel], sc[sel], cl[sel], tb[sel]
        clips.append({"boxes": bx, "scores": sc, "labels": cl, "tubes": tb})
    return clips


def classified_rows(args, prob, flat_tubes, nums, conf_thresh=None):
    """The body of train_cls.py's validate() (:508-543): the classification stage scores the boxes it was GIVEN, so there is no valid_tubes
    and NO NMS -- per clip and class, in tube order, every tube with prob[tube, class] > conf_thresh gives a row: the box of the tube's
    middle frame divided by [W,H,W,H], the class, the score.  prob [N,NC] (a cls_only head's output), flat_tubes [N,Tl,5] (frame-index
    column first) or [N,Tl,4], nums = tubes per clip (host ints).  Returns what postprocess() returns for ONE iteration -- a list over clips of
    {boxes [m,4] fp32 normalised, scores [m], labels [m], tubes [m]} -- so detections_csv and evaluate.FrameMAP.add_detections take it
    unchanged.  One comparison for the keep mask, then the row compaction of postprocess() (step_detect_compact, <= 1024 tubes per clip; the
    nonzero / gather form beyond that) and its one host synchronisation for the row counts."""
    conf = float(getattr(args, "conf_thresh", 0.01) if conf_thresh is None else conf_thresh)
    W, H = float(args.image_size[0]), float(args.image_size[1])
    nums = [int(v) for v in nums]
    dev = prob.device
    B = len(nums)
    if B == 0 or sum(nums) == 0:
        e = torch.zeros(0, device=dev)
        return [{"boxes": e.view(0, 4), "scores": e, "labels": e.long(), "tubes": e.long()} for _ in nums]
    scores = prob.float().contiguous()
    NC = scores.shape[1]
    boxes = flat_tubes[:, int(flat_tubes.shape[1] / 2), -4:].float().contiguous()                     # :515
    idx, valid = _clip_groups(nums, dev)
    kmax = idx.shape[1]
    keep = ((scores[idx].permute(0, 2, 1) > conf) & valid.view(B, 1, kmax)).to(torch.uint8).contiguous()     # [B,NC,kmax] (:520)
    if COMPACT_KERNEL and kmax <= _fused_tubes():
        n = torch.as_tensor(nums, device=dev, dtype=torch.int32)
        start = (torch.cumsum(n, 0) - n).to(torch.int32)
        rb, rs, kc, kj, cnt = ops.detect_compact(keep.view(1, B, NC, kmax), [boxes], [scores], start, W, H)
        per = cnt.tolist()                                                                            # the one host sync
        cap = NC * kmax
        return [{"boxes": rb[b * cap:b * cap + per[b]], "scores": rs[b * cap:b * cap + per[b]], "labels": kc[b * cap:b * cap + per[b]],
                 "tubes": kj[b * cap:b * cap + per[b]]} for b in range(B)]
    kb, kc, kj = torch.nonzero(keep, as_tuple=True)
    tube = idx[kb, kj]
    rb = boxes[tube] / torch.tensor([W, H, W, H], device=dev)                                         # :533-534
    rs = scores[tube, kc]
    per = torch.bincount(kb, minlength=B).tolist()
    return [{"boxes": bx, "scores": sc, "labels": cl, "tubes": tb} for bx, sc, cl, tb in zip(rb.split(per), rs.split(per), kc.split(per), kj.split(per))]


def detections_csv(dets, infos, label_dict=None):
    """The text test.py:210-218 writes for one iteration: `dets` = one entry of postprocess()'s result, infos = per clip
    {'video_name', 'fid'}; label_dict maps class index -> label id (identity + 1 when None)."""
    lines = []
    for d, info in zip(dets, infos):
        bx, sc, cl = d["boxes"].cpu().numpy(), d["scores"].cpu().numpy(), d["labels"].cpu().numpy()
        for k in range(len(sc)):
            lab = int(cl[k]) + 1 if label_dict is None else label_dict[int(cl[k])]
            lines.append("{0},{1:04},{2:.4},{3:.4},{4:.4},{5:.4},{6},{7:.4}\n".format(
                info["video_name"], info["fid"], bx[k, 0], bx[k, 1], bx[k, 2], bx[k, 3], lab, sc[k]))
    return lines


def _merge_segments(seg_boxes, seg_scores, seg_cls, seg_tube, cnt, gthr, etopk, topk):
    """The tail of postprocess_merged for G groups at once: seg_* [G,cap(,4)] fixed-capacity row segments in the reference's row order with
    cnt [G] int32 rows each (on the device) -> one dict per group.  The top-k list order, the merge (ONE step_detect_merge launch) and the
    cluster-major output order are batched tensor operations on the device-side counts; the ONE host copy fetches rows, selected rows
    and clusters per group together, behind the launch."""
    G, cap = seg_scores.shape
    dev = seg_scores.device
    pos = torch.arange(cap, device=dev).view(1, cap)
    order = sel = None
    if etopk > 0:                                                                                     # demo.py:171-174
        # list.sort(key=score) is stable and ascending, then reversed: descending with ties in REVERSED row order == a stable descending
        # sort of the flipped segment; rows past the count sort last
        key = torch.where(pos < cnt.view(G, 1), seg_scores, torch.full_like(seg_scores, float("-inf")))
        order = (cap - 1) - torch.argsort(torch.flip(key, dims=(1,)), dim=1, descending=True, stable=True)
        sel = (cnt.clamp(max=topk) if topk >= 0 else (cnt + topk).clamp(min=0)).to(torch.int32)      # what `[:topk]` keeps
        order32 = order.to(torch.int32)
    cluster, lead_pos, merged, ncl = ops.detect_merge(seg_boxes, cnt, gthr, order32 if order is not None else None, sel)
    # the reference writes cluster after cluster, members in list order (demo.py:210-217): a stable sort of the list positions by cluster
    cl64 = cluster.long()
    perm = torch.argsort(torch.where(cl64 >= 0, cl64, torch.full_like(cl64, cap)), dim=1, stable=True)
    row = perm if order is None else torch.gather(order, 1, perm)
    o_cluster = torch.gather(cl64, 1, perm)
    o_scores, o_cls, o_tube = torch.gather(seg_scores, 1, row), torch.gather(seg_cls, 1, row), torch.gather(seg_tube, 1, row)
    stats = torch.stack([cnt if sel is None else sel, ncl]).tolist()                                  # the one host sync
    return [{"boxes": merged[g, :stats[1][g]], "cluster": o_cluster[g, :stats[0][g]], "labels": o_cls[g, :stats[0][g]],
             "scores": o_scores[g, :stats[0][g]], "tubes": o_tube[g, :stats[0][g]]} for g in range(G)]


def postprocess_merged(args, history, conf_thresh=None, nms_thresh=None, global_thresh=0.8, evaluate_topk=None, topk=None, iterations=None):
    """postprocess() followed by the cross-class merge of demo.py:176-198, which turns a clip's per-class rows into one box per person with
    its list of (action, score): walking the rows in list order (postprocess()'s order), the first row without a cluster leads one, and
    every later row without a cluster whose IoU with the LEADER's box (compute_box_iou on the normalised fp32 boxes) is > global_thresh
    joins it; the cluster's box is the mean of its members' boxes (np.mean: summed in list order).  demo.py:54-55 sets conf_thresh = 0.4
    and global_thresh = 0.8 as locals; here conf_thresh defaults to args.conf_thresh like postprocess().

    Same launches as postprocess() for the mask, NMS and row compaction; then the list order after top-k for all groups as batched tensor
    operations, ONE step_detect_merge launch per set of iterations that share a clip layout, and ONE host synchronisation behind it (rows,
    selected rows and clusters per group in one copy) on the fused path: <= 1024 tubes per clip and NC * kmax <= 65536 rows per segment
    (step_detect_merge's limit); the general path beyond keeps the synchronisation of its nonzero.

    Returns a list over iterations of lists over clips of dicts {boxes [K,4] fp32 normalised merged boxes in cluster order, cluster [m]
    (index into boxes), labels [m], scores [m], tubes [m]}, rows in the order the reference writes them: cluster after cluster, members in
    list order.  Where two clusters of a clip have the same merged box, the reference's dict (keyed by the box's text) keeps only the later
    one; this returns both."""
    conf = float(getattr(args, "conf_thresh", 0.01) if conf_thresh is None else conf_thresh)
    thr = float(getattr(args, "nms_thresh", 0.4) if nms_thresh is None else nms_thresh)
    etopk = int(getattr(args, "evaluate_topk", -1) if evaluate_topk is None else evaluate_topk)
    topk = int(getattr(args, "topk", -1) if topk is None else topk)
    gthr = float(global_thresh)
    W, H = float(args.image_size[0]), float(args.image_size[1])
    todo = [(it, h) for it, h in enumerate(history) if iterations is None or it in iterations]
    out = [None] * len(todo)
    groups = {}
    for oi, (it, h) in enumerate(todo):
        nums = [int(v) for v in h["tubes_nums"]]
        if len(nums) == 0 or sum(nums) == 0:
            e = torch.zeros(0, device=h["pred_loc"].device)
            out[oi] = [{"boxes": e.view(0, 4), "cluster": e.long(), "labels": e.long(), "scores": e, "tubes": e.long()} for _ in nums]
        else:
            groups.setdefault((tuple(nums), h["pred_prob"].shape[-1], h["pred_loc"].device, _count_key(h)), []).append((oi, h))
    for (nums, NC, dev, _), members in groups.items():
        B, kmax = len(nums), max(nums)
        count = members[0][1].get("tubes_count")
        cap = NC * kmax
        if kmax <= 64 or (kmax <= _fused_tubes() and cap <= MERGE_ROWS_MAX):
            for m0 in range(0, len(members), 8):                                                      # (STEP_DETECT_ITERS_MAX iterations per launch)
                part = members[m0:m0 + 8]
                keep, bx_all, sc_all, start, _ = _detect_keep(nums, NC, dev, part, conf, thr, W, H, count)
                rb, rs, kc, kj, cnt = ops.detect_compact(keep, bx_all, sc_all, start, W, H)
                G = len(part) * B
                res = _merge_segments(rb.view(G, cap, 4), rs.view(G, cap), kc.view(G, cap), kj.view(G, cap), cnt, gthr, etopk, topk)
                for k, (oi, h) in enumerate(part):
                    out[oi] = res[k * B:(k + 1) * B]
        elif count is not None:
            raise NotImplementedError("step_amd: a padded history (tubes_count) takes the fused path: at most %d slots per clip and %d rows per segment"
                                      % (_fused_tubes(), MERGE_ROWS_MAX))
        else:
            # the general path's rows come as one flat list per iteration: scatter them into the same fixed-capacity segments
            I = len(members)
            seg_b = torch.zeros((I * B, cap, 4), dtype=torch.float32, device=dev)
            seg_s = torch.zeros((I * B, cap), dtype=torch.float32, device=dev)
            seg_c = torch.zeros((I * B, cap), dtype=torch.int64, device=dev)
            seg_t = torch.zeros((I * B, cap), dtype=torch.int64, device=dev)
            cnts = []
            for k, (oi, h) in enumerate(members):
                kb, kc, rb, rs, rt = _general_rows(h, list(nums), conf, thr, W, H)
                per = torch.bincount(kb, minlength=B)
                at = torch.arange(kb.shape[0], device=dev) - (torch.cumsum(per, 0) - per)[kb]         # row number inside its clip
                g = kb + k * B
                seg_b[g, at], seg_s[g, at], seg_c[g, at], seg_t[g, at] = rb, rs, kc, rt
                cnts.append(per)
            res = _merge_segments(seg_b, seg_s, seg_c, seg_t, torch.cat(cnts).to(torch.int32), gthr, etopk, topk)
            for k, (oi, h) in enumerate(members):
                out[oi] = res[k * B:(k + 1) * B]
    return out


def merged_csv(dets, infos, label_dict=None):
    """The text demo.py:210-217 writes for one batch: `dets` = one entry of postprocess_merged()'s result, infos = per clip {'video_name',
    'fid'}; per cluster, one line per member with the MERGED box; label_dict maps class index -> label id (identity + 1 when None)."""
    lines = []
    for d, info in zip(dets, infos):
        bx, k_, sc, cl = d["boxes"].cpu().numpy(), d["cluster"].cpu().numpy(), d["scores"].cpu().numpy(), d["labels"].cpu().numpy()
        for k in range(len(sc)):
            lab = int(cl[k]) + 1 if label_dict is None else label_dict[int(cl[k])]
            b = bx[k_[k]]
            lines.append("{0},{1:04},{2:.4},{3:.4},{4:.4},{5:.4},{6},{7:.4}\n".format(
                info["video_name"], info["fid"], b[0], b[1], b[2], b[3], lab, sc[k]))
    return lines


class GraphedInference:
    """BaseNet -> ContextNet -> multi-step inference for a FIXED batch size / tubes-per-clip, captured once
    in a hipGraph and replayed: the ~200 small launches of the three refinement steps stop being bound by
    Python / launch latency.  `__call__(images, tubes)` copies the inputs into the captured buffers, replays
    and returns (history, conv_feat, context_feat) -- static tensors that the next call overwrites.

    capacity=K: captured once over B * K padded slots (pad_tubes) with the tubes per clip in a device-side count.  `__call__(images, tubes)`
    then takes ANY list with at most K tubes per clip, zero included (more raises ValueError), without recapture and without host
    synchronisation: slots and counts travel in one non-blocking copy out of two pinned blocks used in turn, each guarded by an event.  The
    history carries "tubes_count"; its rows are slots, a clip's real tubes first."""

    def __init__(self, args, base_net, context_net, nets, images, tubes, capacity=None):
        self.args, self.base, self.ctx, self.nets = args, base_net, context_net, nets
        dev = images.device
        self.images = images.clone()
        self.capacity = None if capacity is None else int(capacity)
        self.count = None
        if self.capacity is not None:
            if self.capacity < 1:
                raise ValueError("step_amd: GraphedInference wants a capacity of at least one tube per clip")
            B, K = len(tubes), self.capacity
            W, H = float(args.image_size[0]), float(args.image_size[1])
            flat, count = pad_tubes(tubes, K, "cpu", W, H)
            self._T, self._whwh = flat.shape[1], (0.0, 0.0, W, H)
            words = flat.numel()
            # slots and counts lie in ONE buffer (the counts' int32 bits behind the slots), so that a call is one copy
            self._slots = torch.empty(words + B, dtype=torch.float32, device=dev)
            self.flat0, self.count = self._slots[:words].view(B * K, self._T, 5), self._slots[words:].view(torch.int32)
            self._stage = [[torch.empty(words + B, dtype=torch.float32).pin_memory(), torch.cuda.Event(), False] for _ in range(2)]
            self._stage_at = 0
            self.nums = [K] * B
            self._write_slots(flat, count)
        else:
            flat, self.nums = _flat_tubes(tubes, dev)
            self.flat0 = flat.clone()
        self.clip_of = torch.as_tensor(np.repeat(np.arange(len(self.nums)), self.nums), device=dev)
        with torch.no_grad():
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(2):                        # warm-up: packs weights, fills caches and the allocator
                    self._run()
            torch.cuda.current_stream(dev).wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = self._run()

    def _run(self):
        cf = self.base(self.images)
        cx = self.ctx(cf) if not self.args.no_context else None
        hist, _ = inference_flat(self.args, cf, cx, self.nets, self.args.max_iter, self.flat0, self.nums, self.clip_of, want_classes=False,
                                 counts=self.count)
        return hist, cf, cx

    def _write_slots(self, flat, count):
        """host (flat [B*K,T,5], count [B] int32) -> the captured buffers, through the next pinned block"""
        st = self._stage[self._stage_at % 2]
        self._stage_at += 1
        if st[2] and not st[1].query():                                        # the copy that last read this block: finished before it is rewritten
            st[1].synchronize()
        words = flat.numel()
        st[0][:words].copy_(flat.reshape(-1))
        st[0][words:].view(torch.int32).copy_(count)
        self._slots.copy_(st[0], non_blocking=True)
        st[1].record(torch.cuda.current_stream(self._slots.device))
        st[2] = True

    def __call__(self, images=None, tubes=None):
        # images: a new clip batch, copied into the captured input buffer -- or None / `self.images` itself when the caller (a decoder, the
        # uint8 -> 16-bit conversion, bench.py's resident-input loop) has written the batch there already: at C3 size the copy is 138 MB
        # read + 138 MB written per step, ~1 % of it
        if images is not None and images.data_ptr() != self.images.data_ptr():
            self.images.copy_(images)
        if tubes is not None and self.capacity is not None:
            if len(tubes) != len(self.nums):
                raise ValueError("step_amd: GraphedInference was captured for %d clips, got %d" % (len(self.nums), len(tubes)))
            self._write_slots(*pad_tubes([np.zeros((0, self._T, 4), np.float32) if len(t) == 0 else t for t in tubes], self.capacity, "cpu",
                                         self._whwh[2], self._whwh[3]))
        elif tubes is not None:
            flat, nums = _flat_tubes(tubes, self.images.device)
            assert nums == self.nums, "GraphedInference was captured for %s tubes per clip" % (self.nums,)
            self.flat0.copy_(flat)
        self.graph.replay()
        return self.out
