"""step_amd/selection.py -- training sample selection between the steps of the progressive head.

Host-side counterpart of the reference's `train_select` / `select_proposals` (utils/utils.py:135-423) and
`compute_tube_iou` / `compute_box_iou` (utils/tube_utils.py:269-351).  The reference walks ground truths x proposals
x frames in interpreted loops; here the IoU table and the target assembly are array operations.  Two things are kept
exactly, because they decide WHICH tubes are trained on:

* the fp32 arithmetic of the IoU (same operations in the same order; the per-tube mean is taken in double and rounded to
  fp32 once, as the reference's Python-float accumulation does), and
* the order of the draws from the global `random` / `numpy.random` streams (one optional `random.shuffle`, then at most
  two `np.random.choice(..., replace=False)`), so that with the same seeds the same proposals are selected
  (tests/golden/selection_golden.npz was recorded from the reference).

All three `temporal_mode`s ("predict": every shipped script; "extrapolate"; "mean") are supported, like step_amd/driver.py.

`sample_anchors` / `cls_select` are the same for the classification pre-training stage (train_cls.py; data/ava_cls.py:200-261): the loader's
rejection sampling around the ground-truth boxes, pinned to the reference's `random` stream (tests/golden/cls_golden.npz), and the per-clip
selection of train_cls.py:263-291.  `DeviceClsSelector` is their opt-in device form (step_anchor_sample + step_select_train).

`DeviceSelector` is the opt-in device form of the same rule (step_select_train, include/step_amd.h): no host synchronisation, static
output shapes, draws from the device-side generator -- its own stream of draws and index-ordered ties, so it selects other tubes than
the reference does under the reference's seeds.  `train_select` stays the default and the one that is pinned to the reference.  Built with
`temporal_modes=("predict", "extrapolate", "mean")` it takes all three modes (step_tube_grow grows the selected rows of the other two);
without the keyword it refuses them, as it always has.
"""
import random

import numpy as np

from .tube_math import extrapolate_tubes, valid_tubes


def read_proposals(path, min_score=0.8):
    """The person detector's proposals of a split (data/ava.py:199-230 get_proposals) -> {video: {frame id: [[x1, y1, x2, y2], ...]}},
    percent boxes as Python floats.  A line is `video,fid,x1,y1,x2,y2,...,score`: the score is the LAST column, whatever stands between;
    lines with score < min_score are dropped (a score of exactly min_score stays), and a box that repeats inside its frame is kept once,
    boxes in first-seen order.  A frame without an entry falls back to the anchor grid in the loader (data/ava.py:342-358)."""
    results = {}
    with open(path) as fin:
        for line in fin.read().splitlines():
            cols = line.split(",")
            if float(cols[-1]) < min_score:
                continue
            box = [float(v) for v in cols[2:6]]
            boxes = results.setdefault(cols[0], {}).setdefault(int(cols[1]), [])
            if box not in boxes:
                boxes.append(box)
    return results


def box_iou(a, b):
    """IoU table [len(a), len(b)] of boxes [x1,y1,x2,y2] without the +1 pixel convention (tube_utils.py:269-306):
    zero unless both overlap extents are positive; degenerate pairs divide by zero like the reference (nan / inf)."""
    a = np.asarray(a, np.float32).reshape(-1, 4)[:, None, :]
    b = np.asarray(b, np.float32).reshape(-1, 4)[None, :, :]
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), np.float32(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), np.float32(0))
    inter = np.where((iw > 0) & (ih > 0), iw * ih, np.float32(0))
    union = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / union).astype(np.float32)


def tube_iou(t1, t2):
    """[n1, n2] mean over the T frames of the per-frame box IoU; a pair contributes zeros when either whole tube sums
    to zero (the padding convention of tube_utils.py:308-351)."""
    t1 = np.asarray(t1, np.float32)
    t2 = np.asarray(t2, np.float32)
    if t1.ndim < 3:
        t1 = t1.reshape(1, -1, 4)
    if t2.ndim < 3:
        t2 = t2.reshape(1, -1, 4)
    if t1.shape[1] != t2.shape[1]:
        raise AssertionError("Tube with different length!")
    T = t1.shape[1]
    live = np.array([bool(np.sum(t)) for t in t1])[:, None] & np.array([bool(np.sum(t)) for t in t2])[None, :]
    acc = np.zeros((t1.shape[0], t2.shape[0]), np.float64)
    for t in range(T):                                              # frame by frame: the double sum runs in the same order
        acc += np.where(live, box_iou(t1[:, t], t2[:, t]).astype(np.float64), 0.0)
    if T > 0:
        acc /= T
    return acc.astype(np.float32)


def select_proposals(gt_tubes, anchors, scores=None, cls_thresh=0.2, max_pos_num=5, sampling="random", neg_ratio=2, ious=None):
    """-> (positives [(gt, proposal)], negatives [(gt, proposal)], iou table) -- utils/utils.py:341-423.
    Positives: the best free proposal of every ground truth (highest-IoU ground truth first), then random ones among the
    proposals above cls_thresh; negatives: drawn from the rest, uniformly / by score / by softmax(score)."""
    if ious is None:                                                # (the device front end hands the table in: step_select_prepare)
        ious = tube_iou(np.asarray(gt_tubes)[:, :, :4], anchors)
    G, A = ious.shape
    if scores is None:
        scores = ious.max(axis=0)
    taken = set()
    pos = []
    left = ious.copy()
    for _ in range(G):
        g = int(np.argmax(left.max(axis=1)))
        for a in np.argsort(ious[g, :])[::-1]:
            if int(a) not in taken:
                taken.add(int(a))
                pos.append((g, int(a)))
                left[g, :] = -1
                break
    if len(pos) > max_pos_num:
        random.shuffle(pos)
        pos = pos[:max_pos_num]
    above = [int(a) for a in np.where(np.sum(ious > cls_thresh, axis=0))[0] if int(a) not in taken]
    if above and len(pos) < max_pos_num:
        owner = np.argmax(ious[:, above], axis=0)
        draw = np.random.choice(len(above), min(len(above), max_pos_num - len(pos)), p=np.ones((len(above),)) / len(above),
                                replace=False)
        for d in draw:
            taken.add(above[d])
            pos.append((int(owner[d]), above[d]))
            if len(pos) == max_pos_num:
                break
    pos = pos[:max_pos_num]
    taken.update(above)                                             # never a negative: they overlap some ground truth
    rest = [a for a in range(A) if a not in taken]
    neg = []
    if rest:
        w = np.asarray(scores)[rest]
        if sampling == "uniform":
            w = (w + 1e-6) / np.sum(w + 1e-6)
        elif sampling == "random":
            w = np.ones((len(rest),)) / len(rest)
        elif sampling == "softmax":
            w = np.exp(w) / np.sum(np.exp(w))
        else:
            raise NotImplementedError(sampling)
        for d in np.random.choice(len(rest), min(len(pos) * neg_ratio, len(rest)), p=w, replace=False):
            neg.append((int(np.argmax(ious[:, rest[d]])), rest[d]))
    if neg_ratio > 0:
        pos = pos[:max(max_pos_num, int(len(neg) / neg_ratio))]
    return pos, neg, ious


def _top_candidates(prob, topk, num_classes):
    """Rows of the clip's predictions to keep, best first, with their scores: per class the best 2*topk/num_classes tubes
    (all when topk <= 0), merged by score, one entry per tube (utils/utils.py:179-214)."""
    per_cls_idx, per_cls_score = [], []
    keep = int(topk / num_classes) * 2 if topk > 0 else None
    for c in range(num_classes):
        s = prob[:, c].reshape(-1)
        order = np.argsort(s)[::-1]
        per_cls_idx.append(order[:keep])
        per_cls_score.append(s[order][:keep])
    flat_s = np.concatenate(per_cls_score)
    flat_i = np.concatenate(per_cls_idx)
    # ascending stable sort, reversed: what list.sort(key=score)[::-1] yields, ties included
    seen, rows, sc = set(), [], []
    for k in np.argsort(flat_s, kind="stable")[::-1]:
        i = int(flat_i[k])
        if i not in seen:
            seen.add(i)
            rows.append(i)
            sc.append(flat_s[k])
    if topk > 0:
        rows, sc = rows[:topk], sc[:topk]
    return np.asarray(rows, np.int64), np.asarray(sc)


def train_select(step, history, targets, tubes, args, device=None):
    """-> (selected_tubes, target_tubes), one array per clip -- utils/utils.py:135-339.

    step 1 trains on the initial proposals `tubes[b]`; later steps on the best-scoring refined tubes of the previous step
    (`history`: pred_prob [N,T,C], pred_loc [N,T,4], pred_first_loc / pred_last_loc [N,T,4], tubes_nums).  Every selected tube
    comes with one target row per loss frame [first neighbour, centre, last neighbour], each
    [x1,y1,x2,y2, cls flag, reg flag, class labels...].

    device=True (default when the history lives on a ROCm device): the per-tube arithmetic -- class scores averaged over the frames,
    valid_tubes of the three predicted tubes, the IoU table against the clip's ground truths -- is ONE launch (step_select_prepare) and
    ONE device-to-host copy of its small results instead of four copies of the raw predictions and numpy passes over them; the
    sorts and the draws from the random streams, which decide WHICH tubes are trained on, stay here.  Same selections, bit for bit."""
    if args.temporal_mode not in ("predict", "extrapolate", "mean"):
        raise NotImplementedError("temporal_mode %r" % (args.temporal_mode,))
    if history is not None and history.get("tubes_count") is not None:
        raise ValueError("train_select: a padded history (tubes_count) belongs to the device selection (DeviceSelector.select(clip_count=...)); "
                         "the host selection keeps its ragged form")
    chunks, max_chunks = args.NUM_CHUNKS[step], args.NUM_CHUNKS[args.max_iter]
    T = args.T
    t_start = int((max_chunks - chunks) / 2) * T
    t_len = chunks * T
    mid = int(max_chunks / 2)
    cls_thresh, reg_thresh = args.cls_thresh[step - 1], args.reg_thresh[step - 1]
    W, H = args.image_size[0], args.image_size[1]
    nc = args.num_classes
    predict = args.temporal_mode == "predict"
    grow = (step - 1) in args.NUM_CHUNKS and args.NUM_CHUNKS[step] == args.NUM_CHUNKS[step - 1] + 2
    grows_next = predict and step < args.max_iter and args.NUM_CHUNKS[step + 1] == args.NUM_CHUNKS[step] + 2

    def host(x):
        return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)

    dev_path = None
    if step > 1:
        bounds = np.concatenate(([0], np.cumsum(history["tubes_nums"]))).astype(np.int64)
        on_dev = hasattr(history["pred_prob"], "is_cuda") and history["pred_prob"].is_cuda
        if device if device is not None else on_dev:
            dev_path = _prepare_on_device(history, targets, mid, predict, W, H)
        else:
            prob, loc = host(history["pred_prob"]), host(history["pred_loc"])
            first = host(history["pred_first_loc"]) if predict else None
            last = host(history["pred_last_loc"]) if predict else None

    selected, wanted = [], []
    for b in range(len(targets)):
        gt = np.asarray(targets[b])
        if step == 1:
            cand, cand_score, cand_first, cand_last = np.asarray(tubes[b]), None, None, None
        else:
            lo, hi = bounds[b], bounds[b + 1]
            if dev_path is not None:
                mean_prob, vloc, vfirst, vlast, iou_all = dev_path
                rows, cand_score = _top_candidates(mean_prob[lo:hi], args.topk, nc)
                cand = vloc[lo:hi][rows]
                cand_first = vfirst[lo:hi][rows] if predict else None
                cand_last = vlast[lo:hi][rows] if predict else None
                table = np.ascontiguousarray(iou_all[lo:hi][rows][:, :gt.shape[0]].T)            # [G, candidates]
            else:
                rows, cand_score = _top_candidates(prob[lo:hi].mean(axis=1), args.topk, nc)
                cand = valid_tubes(loc[lo:hi][rows], W, H)
                cand_first = valid_tubes(first[lo:hi][rows], W, H) if predict else None
                cand_last = valid_tubes(last[lo:hi][rows], W, H) if predict else None
        pos, neg, ious = select_proposals(gt[:, mid].reshape(gt.shape[0], 1, -1), cand[:, int(cand.shape[1] / 2)].reshape(cand.shape[0], 1, -1),
                                          cand_score, cls_thresh, args.max_pos_num, args.selection_sampling, args.neg_ratio,
                                          ious=table if (step > 1 and dev_path is not None) else None)
        pg = np.asarray([g for g, _ in pos], np.int64)
        pa = np.asarray([a for _, a in pos], np.int64)
        ng = np.asarray([g for g, _ in neg], np.int64)
        na = np.asarray([a for _, a in neg], np.int64)
        rows_a = np.concatenate((pa, na))
        R, P = len(rows_a), len(pa)
        sel = cand[rows_a].astype(np.float32).reshape(R, cand.shape[1], 4)
        centre = np.zeros((R, 1, 6 + nc), np.float32)
        centre[:P, 0, :4] = gt[pg, mid, :4]
        centre[:P, 0, 6:] = gt[pg, mid, 4:]
        centre[:P, 0, 4:6] = 1                                      # positives: classification and regression
        reg_only = ious[ng, na] >= reg_thresh if len(ng) else np.zeros((0,), bool)
        centre[P:, 0, :4][reg_only] = gt[ng[reg_only], mid, :4]     # negatives close enough to a ground truth still regress
        centre[P:, 0, 6:][reg_only] = gt[ng[reg_only], mid, 4:]
        centre[P:, 0, 5][reg_only] = 1
        if grow:
            if predict:
                sel = np.concatenate((cand_first[rows_a].astype(np.float32).reshape(R, T, 4), sel,
                                      cand_last[rows_a].astype(np.float32).reshape(R, T, 4)), axis=1)
            elif args.temporal_mode == "extrapolate":
                sel = extrapolate_tubes(sel, T)
            else:
                m = np.tile(np.mean(sel, axis=1, keepdims=True), (1, T, 1))
                sel = np.concatenate((m, sel, m), axis=1)
        before = np.zeros((R, 1, 6 + nc), np.float32)
        after = np.zeros((R, 1, 6 + nc), np.float32)
        if grows_next and P:
            for dst, frame in ((before, int((t_start - T) / T)), (after, int((t_start + t_len) / T))):
                dst[:P, 0, :4] = gt[pg, frame, :4]
                dst[:P, 0, 5] = dst[:P, 0, :4].sum(axis=1) > 0       # an all-zero box is padding: no regression target
                dst[:P, 0, 6:] = gt[pg, frame, 4:]
        selected.append(sel)
        wanted.append(np.concatenate((before, centre, after), axis=1))
    return selected, wanted


def _prepare_on_device(history, targets, mid, predict, W, H):
    """step_select_prepare over a step's predictions (device tensors) -> host arrays (mean_prob [N,NC], vloc [N,T,4], vfirst / vlast
    [N,Tw,4] | None, iou [N,Gmax]) through one packed device-to-host copy."""
    import torch

    from . import ops
    prob = history["pred_prob"]
    dev = prob.device
    nums = [int(v) for v in history["tubes_nums"]]
    B = len(nums)
    Gmax = max([np.asarray(t).shape[0] for t in targets] + [1])
    gt = np.zeros((B, Gmax, 4), np.float32)
    cnt = np.zeros((B,), np.int32)
    for b, t in enumerate(targets):
        t = np.asarray(t)
        cnt[b] = t.shape[0]
        gt[b, :t.shape[0]] = t[:, mid, :4]
    clip_of = torch.as_tensor(np.repeat(np.arange(B), nums).astype(np.int32), device=dev)
    outs = ops.select_prepare(prob, history["pred_loc"], history["pred_first_loc"] if predict else None,
                              history["pred_last_loc"] if predict else None, clip_of, torch.from_numpy(gt).to(dev), torch.from_numpy(cnt).to(dev),
                              float(W), float(H))
    sizes = [o.numel() for o in outs if o is not None]
    packed = torch.cat([o.reshape(-1) for o in outs if o is not None]).cpu().numpy()           # the one device-to-host copy
    res, k, off = [], 0, 0
    for o in outs:
        if o is None:
            res.append(None)
            continue
        res.append(packed[off:off + sizes[k]].reshape(tuple(o.shape)))
        off += sizes[k]
        k += 1
    return res


class DeviceSelector:
    """train_select for a FIXED batch on the device: select(step, ...) is step_select_prepare (step > 1) + step_select_train on the
    current stream, into static buffers -- nothing is copied to the host, nothing waits, so the calls can be recorded in a graph and the
    draws (step_amd.rng.DeviceRNG: one offset per select()) change from replay to replay.

    temporal_modes: the allow-list of args.temporal_mode values this selector may be built for.  The default is ("predict",): the
    selector was written for that mode alone, callers (and tests/select_cases.py) rely on the positional form refusing the other two
    with NotImplementedError before any launch, and a caller that never asked for them should keep falling back to the host selection
    rather than silently change path.  temporal_modes=("predict", "extrapolate", "mean") admits all three: outside "predict" the step
    that grows the tubes selects the un-grown rows (step_select_train without neighbour candidates, into a scratch buffer) and grows
    the selected rows from their own boxes (step_tube_grow), as train_select does -- without valid_tubes after the growth, like it --
    and no step writes neighbour targets."""

    ALL_MODES = ("predict", "extrapolate", "mean")

    def __init__(self, args, batch, budget, device, rng, dynamic_gt=False, temporal_modes=("predict",)):
        import torch
        if args.temporal_mode not in temporal_modes or args.temporal_mode not in self.ALL_MODES:
            raise NotImplementedError("DeviceSelector: temporal_mode %r stays on the host path (selection.train_select) unless temporal_modes= "
                                      "admits it" % (args.temporal_mode,))
        if args.selection_sampling not in ("uniform", "random", "softmax"):
            raise NotImplementedError(args.selection_sampling)
        if budget < args.max_pos_num * (1 + args.neg_ratio):
            raise ValueError("DeviceSelector: budget %d is below max_pos_num * (1 + neg_ratio) = %d" % (budget, args.max_pos_num * (1 + args.neg_ratio)))
        self.args, self.batch, self.budget, self.device, self.rng = args, int(batch), int(budget), torch.device(device), rng
        K, nc = self.batch * self.budget, args.num_classes
        self._layout = None                                      # (key, clip_of, most tubes of one clip) of the clip_start last seen
        self._gt_mid = None                                      # (key, the ground truths' middle-frame boxes, dense)
        # dynamic_gt: the ground truths change UNDER the selector -- a kernel writes them through a raw pointer (step_augment_plan's gt_out),
        # which bumps no tensor version -- so the middle-frame gather is issued on every select() (and recorded with it in a graph)
        self.dynamic_gt = bool(dynamic_gt)
        self.out = {}
        self._ungrown = {}                                       # outside "predict": the growing steps' selected rows before step_tube_grow
        self._slot_clip = torch.arange(self.batch, dtype=torch.int32, device=self.device).repeat_interleave(self.budget)
        for i in range(1, args.max_iter + 1):
            Tl = args.NUM_CHUNKS[i] * args.T
            self.out[i] = (torch.zeros((K, Tl, 5), device=self.device), torch.zeros((K, 3, 6 + nc), device=self.device),
                           torch.zeros((K, 1), device=self.device), torch.zeros((1,), device=self.device),
                           torch.zeros((self.batch, 2), dtype=torch.int32, device=self.device))
            if args.temporal_mode != "predict" and (i - 1) in args.NUM_CHUNKS and args.NUM_CHUNKS[i] == args.NUM_CHUNKS[i - 1] + 2:
                self._ungrown[i] = torch.zeros((K, Tl - 2 * args.T, 5), device=self.device)

    @staticmethod
    def _key(t):
        return (t.data_ptr(), t._version, tuple(t.shape))

    def _clip_layout(self, clip_start):
        """(clip_of [N] int32, most tubes of one clip) of a clip_start table; read once per table (one small copy to the host) and again
        whenever another tensor, or the same one written to since, is handed in -- so not inside a graph capture, where the first
        select() of a table must not fall"""
        import torch
        key = self._key(clip_start)
        if self._layout is None or self._layout[0] != key:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceSelector: a new clip_start table cannot be read inside a graph capture (run select() once before capturing)")
            nums = (clip_start[1:] - clip_start[:-1]).cpu().numpy().astype("int64")
            clip_of = torch.as_tensor(np.repeat(np.arange(len(nums)), nums).astype(np.int32), device=self.device)
            self._layout = (key, clip_of, int(nums.max()) if len(nums) else 0)
        return self._layout[1], self._layout[2]

    def _gt_mid_boxes(self, gt, mid):
        """gt[:, :, mid, :4] as the dense tensor step_select_prepare reads; made again only when gt was replaced or written to"""
        if self.dynamic_gt:
            return gt[:, :, mid, :4].contiguous()
        key = self._key(gt) + (mid,)
        if self._gt_mid is None or self._gt_mid[0] != key:
            self._gt_mid = (key, gt[:, :, mid, :4].contiguous())
        return self._gt_mid[1]

    def select(self, step, history, gt, gt_count, init_flat, clip_start, pad_tubes, max_tubes=None, clip_count=None):
        """history: the previous step's predictions (driver.inference_flat's entry; None at step 1); gt [B,Gmax,F,4+NC], gt_count [B]
        int32, init_flat [N,T,4] the initial tubes (step 1's candidates), clip_start [B+1] int32, pad_tubes [B,Tl,4] of THIS step -- all
        on the device.  max_tubes: the most tubes of one clip (default: read from clip_start the first time the table is seen).
        clip_count [B] int32 | None: padded clips -- clip_start describes the SLOTS, the first clip_count[b] of clip b's are real tubes
        (step_select_train_counted; step_select_prepare runs over all slots).  -> (sel, tgt, mask, inv, counts), the step's static buffers."""
        from . import ops
        a = self.args
        chunks, max_chunks = a.NUM_CHUNKS[step], a.NUM_CHUNKS[a.max_iter]
        T = a.T
        t_start = int((max_chunks - chunks) / 2) * T
        mid = int(max_chunks / 2)
        grow = (step - 1) in a.NUM_CHUNKS and a.NUM_CHUNKS[step] == a.NUM_CHUNKS[step - 1] + 2
        predict = a.temporal_mode == "predict"
        grows_next = predict and step < a.max_iter and a.NUM_CHUNKS[step + 1] == a.NUM_CHUNKS[step] + 2      # (neighbour targets: "predict" only)
        before, after = (int((t_start - T) / T), int((t_start + chunks * T) / T)) if grows_next else (-1, -1)
        clip_of, most = self._clip_layout(clip_start)
        if step == 1:
            cand, first, last, score, iou = init_flat, None, None, None, None
        else:
            nbr = grow and predict                               # (the other modes' histories carry None for the neighbours)
            score, cand, first, last, iou = ops.select_prepare(history["pred_prob"], history["pred_loc"], history["pred_first_loc"] if nbr else None,
                                                               history["pred_last_loc"] if nbr else None, clip_of, self._gt_mid_boxes(gt, mid),
                                                               gt_count, float(a.image_size[0]), float(a.image_size[1]))
        n_max = int(max_tubes) if max_tubes is not None else most
        out = self.out[step]
        if grow and not predict:
            # the selected rows grow from their own boxes: step_select_train writes them un-grown (its pad: the middle frames of the step's),
            # step_tube_grow makes the step's sel of them -- the padded slots get the step's pad, the index column is rewritten for Tl frames
            Tc = cand.shape[1]
            mid_pad = pad_tubes[:, T:T + Tc].contiguous()
            ops.select_train(cand, None, None, score, iou, clip_start, n_max, gt, gt_count, mid_pad, self.rng, mid, before, after, a.topk,
                             a.cls_thresh[step - 1], a.reg_thresh[step - 1], a.max_pos_num, a.neg_ratio, a.selection_sampling, self.budget,
                             out=(self._ungrown[step],) + tuple(out[1:]), clip_count=clip_count)
            ops.tube_grow(self._ungrown[step], T, a.temporal_mode, self._slot_clip, mask=out[2], pad_tubes=pad_tubes, out=out[0])
            return out
        return ops.select_train(cand, first, last, score, iou, clip_start, n_max, gt, gt_count, pad_tubes, self.rng, mid, before, after, a.topk,
                                a.cls_thresh[step - 1], a.reg_thresh[step - 1], a.max_pos_num, a.neg_ratio, a.selection_sampling, self.budget,
                                out=out, clip_count=clip_count)


# ---- classification pre-training (train_cls.py: stage 1 of the reference's two-stage recipe) --------------------------------------------
def _jaccard(boxes, box):
    """IoU of every row of boxes [G,4] with one box [4] in the arithmetic of data/augmentations.py:15-39: intersection sides clamped below at
    0, union = area + area - intersection; no guard against a zero union."""
    hi = np.minimum(boxes[:, 2:], box[2:])
    lo = np.maximum(boxes[:, :2], box[:2])
    side = np.clip(hi - lo, a_min=0, a_max=np.inf)
    inter = side[:, 0] * side[:, 1]
    union = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) + (box[2] - box[0]) * (box[3] - box[1]) - inter
    return inter / union


def _centred(cx, cy, bw, bh):
    return np.array([cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh], dtype=float)


def sample_anchors(anchors, pos_num=1, neg_ratio=1, pos_thresh=0.75, neg_thresh=0.2, mode='train'):
    """-> [rows, 4]: per box of `anchors` ([G,4], normalised to [0, 1]) its sampled positives -- or the box itself when none was found, and
    always outside mode 'train' -- followed by its sampled negatives (data/ava_cls.py:200-261).

    Train mode first tries up to 50 boxes of 0.8-1.2 times the size within 0.2 of the centre: one that overlaps its own box by more than
    pos_thresh and every other box by less than neg_thresh is a positive, one below neg_thresh everywhere a negative; the loop ends with the
    pos_num-th positive.  Then, in both modes, up to 50 boxes of 0.3-0.7 or 1.5-2 times the size, shifted by 0.3-1 of it, fill the negatives
    up to pos_num * neg_ratio.  Every draw is one call of `random.uniform` / `random.choice` in the reference's order (both options of a
    choice are drawn before the choice; the loop that fills the negatives draws one whole trial even when nothing is missing), so that with
    the same `random` seed the same boxes come out, bit for bit in float64, and the stream is left where the reference leaves it."""
    want_neg = pos_num * neg_ratio
    uni, pick = random.uniform, random.choice
    rows = []
    for i in range(anchors.shape[0]):
        box = anchors[i]
        w = box[2] - box[0]
        h = box[3] - box[1]
        x = box[0] + 0.5 * w
        y = box[1] + 0.5 * h
        pos, neg = [], []

        def is_negative(c):
            iou = _jaccard(anchors, c)
            return (iou < neg_thresh).sum() == iou.shape[0]

        if mode == 'train':
            for _ in range(50):
                bw = uni(0.8 * w, min(1, 1.2 * w))
                bh = uni(0.8 * h, min(1, 1.2 * h))
                cx = uni(max(0.5 * bw, x - 0.2 * w), min(1 - 0.5 * bw, x + 0.2 * w))
                cy = uni(max(0.5 * bh, y - 0.2 * h), min(1 - 0.5 * bh, y + 0.2 * h))
                c = _centred(cx, cy, bw, bh)
                iou = _jaccard(anchors, c)
                below = (iou < neg_thresh).sum()
                if len(pos) < pos_num and iou[i] > pos_thresh and below == iou.shape[0] - 1:
                    pos.append(c)
                elif len(neg) < want_neg and below == iou.shape[0]:
                    neg.append(c)
                if len(pos) == pos_num:
                    break
        else:
            pos.append(box)
        for _ in range(50):
            bw = pick((uni(0.3 * w, 0.7 * w), min(1, uni(1.5 * w, 2 * w))))
            bh = pick((uni(0.3 * h, 0.7 * h), min(1, uni(1.5 * h, 2 * h))))
            cx = pick((uni(max(0.5 * bw, x - w), max(0.5 * bw, x - 0.3 * w)), uni(min(1 - 0.5 * bw, x + 0.3 * w), min(1 - 0.5 * bw, x + w))))
            # (x - h below is the reference's rule, ava_cls.py:242: the distribution of the negatives follows it)
            cy = pick((uni(max(0.5 * bh, x - h), max(0.5 * bh, y - 0.3 * h)), uni(min(1 - 0.5 * bh, y + 0.3 * h), min(1 - 0.5 * bh, y + h))))
            c = _centred(cx, cy, bw, bh)
            if len(neg) < want_neg and is_negative(c):
                neg.append(c)
            if len(neg) == want_neg:
                break
        rows.extend(pos if pos else [box])
        rows.extend(neg)
    return np.stack(rows, axis=0)


def cls_select(targets, tubes, args=None):
    """The per-clip body of train_cls.py:263-291 -> (selected_tubes, target_tubes), one array per clip: select_proposals on the middle frames
    (cls_thresh 0.75, at most 5 positives, negatives by IoU-weighted draws, 3 per positive; draws from `random` / `numpy.random` in the
    reference's order), the selected tubes [n,T,4] fp32 and the targets [n,3,6+NC]: a positive carries its ground truth's box and labels, a
    negative zeros; column 4 (the classification flag) is 1 on every row; the one row is repeated for the three loss frames."""
    selected, wanted = [], []
    for b in range(len(targets)):
        gt, cur = np.asarray(targets[b]), np.asarray(tubes[b])
        nc = gt.shape[2] - 4
        if args is not None and nc != args.num_classes:
            raise ValueError("cls_select: targets carry %d classes, args.num_classes is %d" % (nc, args.num_classes))
        mid = 0                                                     # int(max_chunks / 2) with max_chunks = 1
        pos, neg, _ = select_proposals(gt[:, mid].reshape(gt.shape[0], 1, -1), cur[:, int(cur.shape[1] / 2)].reshape(cur.shape[0], 1, -1),
                                       None, 0.75, 5, "uniform", 3)
        n = len(pos) + len(neg)
        sel = np.zeros((n, cur.shape[1], 4), np.float32)
        row = np.zeros((n, 1, 6 + nc), np.float32)
        for r, (g, a) in enumerate(pos + neg):
            sel[r] = cur[a]
            if r < len(pos):
                row[r, :, :4] = gt[g, mid, :4]
                row[r, :, 6:] = gt[g, mid, 4:]
        row[:, :, 4] = 1
        selected.append(sel)
        wanted.append(np.concatenate([row, row, row], axis=1))
    return selected, wanted


class DeviceClsSelector:
    """sample_anchors + cls_select for a FIXED batch on the device (opt-in): select() is step_anchor_sample followed by step_select_train
    (score and iou NULL: the candidates are the sampled tubes, the table is the kernel's own) on the current stream, into static buffers --
    two launches and two offsets of `rng` per iteration (and one strided copy of the row mask into the targets' flag column), nothing returned
    to the host, so the calls can be recorded in a graph and draw anew
    on every replay.  The draws are the device generator's, not the reference's.  cls_thresh 0.75, at most 5 positives, 3 negatives per
    positive, weights IoU + 1e-6 (train_cls.py:266-270); reg_thresh is above 1, so no negative gets a box or labels; budget 20 slots per
    clip.  Two differences from cls_select's targets, neither of which a cls_only head reads (it takes targets[:, 1] and its flag and label
    columns only): the device form writes the CENTRE row alone -- rows 0 and 2, which the host form fills with copies of it, stay zero --
    and column 5 of a positive's centre row (the regression flag) is 1 where the host form leaves 0."""
    CLS_THRESH, MAX_POS, NEG_RATIO, BUDGET = 0.75, 5, 3, 20

    def __init__(self, args, batch, Gmax, dev, rng, pos_num=1, neg_ratio=3, mode="train"):
        import torch
        self.args, self.batch, self.Gmax, self.device, self.rng = args, int(batch), int(Gmax), torch.device(dev), rng
        self.pos_num, self.neg_ratio, self.mode = int(pos_num), int(neg_ratio), mode
        self.chunks = args.NUM_CHUNKS[1]
        self.T = args.T * self.chunks
        self.budget = self.BUDGET
        S = self.pos_num * (1 + self.neg_ratio)
        K, nc, d = self.batch * self.budget, args.num_classes, self.device
        self.sampled = (torch.zeros((self.batch * self.Gmax * S, self.T, 4), device=d), torch.zeros((self.batch + 1,), dtype=torch.int32, device=d),
                        torch.zeros((self.batch * self.Gmax, 2), dtype=torch.int32, device=d))
        self.out = (torch.zeros((K, self.T, 5), device=d), torch.zeros((K, 3, 6 + nc), device=d), torch.zeros((K, 1), device=d),
                    torch.zeros((1,), device=d), torch.zeros((self.batch, 2), dtype=torch.int32, device=d))

    def select(self, gt, gt_count, pad_tubes):
        """gt [B,Gmax,chunks,4+NC] float32 pixel boxes, gt_count [B] int32, pad_tubes [B,T,4] (the box of the padded slots), on the device
        -> (sel [B*20,T,5], tgt [B*20,3,6+NC], mask [B*20,1], inv [1], counts [B,2]), the static buffers."""
        from . import ops
        a = self.args
        if tuple(gt.shape[:3]) != (self.batch, self.Gmax, self.chunks):
            raise RuntimeError("DeviceClsSelector: gt wants [B=%d,Gmax=%d,chunks=%d,4+NC], got %s" % (self.batch, self.Gmax, self.chunks, tuple(gt.shape)))
        mid = self.chunks // 2
        tubes, clip_start, _ = ops.anchor_sample(gt, gt_count, self.rng, mid, float(a.image_size[0]), float(a.image_size[1]), self.T, self.pos_num,
                                                 self.neg_ratio, 0.75, 0.2, self.mode, out=self.sampled)
        S = self.pos_num * (1 + self.neg_ratio)
        out = ops.select_train(tubes, None, None, None, None, clip_start, self.Gmax * S, gt, gt_count, pad_tubes, self.rng, mid, -1, -1, -1,
                               self.CLS_THRESH, 2.0, self.MAX_POS, self.NEG_RATIO, "uniform", self.budget, out=self.out)
        # train_cls.py:278,283 sets the classification flag on EVERY selected row (step_select_train: on the positives): one strided copy of
        # the row mask into column 4 of the centre rows, stream-ordered like the two launches
        out[1][:, 1, 4].copy_(out[2][:, 0])
        return out
