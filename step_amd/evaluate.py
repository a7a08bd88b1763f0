"""step_amd/evaluate.py -- frame-mAP on the device: what the reference's `ava_evaluation` (utils/eval_utils.py:12-23, called at
test.py:225, train.py:580, train_cls.py:551) computes with the vendored ActivityNet `PascalDetectionEvaluator`
(external/ActivityNet/Evaluation), restated for this package.

Semantics (all float64): rows of classes outside the label map and of excluded image keys are dropped; detections with
`not (y1 < y2 and x1 < x2)` are removed; per image and class the detections in descending score order each look at the FIRST ground-truth
box of the largest IoU, and are true positives where that IoU >= 0.5 and no detection of higher rank took the box; per class the rows of all
images in descending score order give precision / recall and the VOC average precision; mAP is the mean over the classes with ground truth.
Ties of equal scores, which the reference leaves to an unstable sort, are defined here as a stable ascending sort, reversed: the LATER row
first -- inside an (image, class) list and inside a class's list over the images (images in the order their detections were added).

The labelling (step_eval_match) and the precision / recall / AP of all classes (step_eval_ap) are one launch each; evaluate() makes one
host synchronisation.  There is no CPU fallback: the tensors live on a ROCm device."""
import math
import re
import warnings

import numpy as np
import torch

from . import ops

GT_ROWS_MAX = 1024                     # ground-truth rows of one image (step_eval_match keeps them in LDS)
DETS_PER_CLASS_MAX = 10000             # object_detection_evaluation.py:466 nms_max_output_boxes: the reference would cut the list there
# the file names ava_evaluation looks for under `root` (the reference's: utils/eval_utils.py:12-23)
AVA_FILES = {"labelmap": "ava_action_list_v2.1_for_activitynet_2018.pbtxt", "exclusions": "ava_val_excluded_timestamps_v2.1.csv",
             "groundtruth": "ava_val_v2.1.csv"}
SCORE_MIN = -10.0                      # np_box_list_ops.py:196-208: the reference drops scores <= -10


def image_key(video, timestamp):
    """the key an image goes by: video name and the timestamp (an integer, or its text) as four digits at least, joined by a comma --
    the form the reference's evaluator keys its images by, so that keys from files and keys from `infos` meet"""
    return ",".join((str(video), format(int(timestamp), "04d")))


def _lines(file):
    if isinstance(file, str):
        with open(file, "r") as f:
            return f.read().splitlines()
    return [ln.rstrip("\r\n") for ln in file]


_LABELMAP_ENTRY = re.compile(r'name\s*:\s*"(?P<name>[^"]*)"[^{}]*?\b(?:label_id|id)\s*:\s*(?P<id>\d+)')


def read_labelmap(file):
    """A label map in the pbtxt form of ava_action_list_v2.1_for_activitynet_2018.pbtxt -> (categories: list of {"id", "name"} in file
    order, class_ids: set of the ids).  One regular expression over the whole text: every `name: "..."` with the `id: n` (or
    `label_id: n`) that follows it inside the same item; indentation and line breaks do not matter.  file: a path or an open text file."""
    text = "\n".join(_lines(file))
    categories = [{"id": int(m.group("id")), "name": m.group("name")} for m in _LABELMAP_ENTRY.finditer(text)]
    return categories, {c["id"] for c in categories}


def read_exclusions(file):
    """A CSV of `video,timestamp` rows -> the set of excluded image keys (None -> empty set)."""
    out = set()
    if file is None:
        return out
    for line in _lines(file):
        if not line.strip():
            continue
        row = line.split(",")
        if len(row) != 2:
            raise ValueError("expected 2 columns, got: %r" % line)
        out.add(image_key(row[0], row[1]))
    return out


def read_ava_csv(file, class_whitelist=None):
    """A CSV in the AVA format, `video,timestamp,x1,y1,x2,y2,action_id[,score]` -> (boxes, labels, scores): dicts from image key to the
    rows of that image in file order, boxes as [x1, y1, x2, y2] floats (every number through float(), as the reference parses them),
    labels as ints, scores 1.0 where the file has no eighth column.  Rows whose action_id is not in class_whitelist are skipped."""
    boxes, labels, scores = {}, {}, {}
    for line in _lines(file):
        if not line.strip():
            continue
        row = line.split(",")
        if len(row) not in (7, 8):
            raise ValueError("wrong number of columns: %r" % line)
        key = image_key(row[0], row[1])
        box = [float(v) for v in row[2:6]]
        action = int(row[6])
        if class_whitelist and action not in class_whitelist:
            continue
        boxes.setdefault(key, []).append(box)
        labels.setdefault(key, []).append(action)
        scores.setdefault(key, []).append(float(row[7]) if len(row) == 8 else 1.0)
    return boxes, labels, scores


class FrameMAP:
    """The PASCAL frame-mAP evaluator of the reference on the device.

        ev = FrameMAP(categories, device="cuda")
        ev.add_groundtruth_csv(gt_file, exclusions)
        ev.add_detections(postprocess(args, history)[-1], infos, args.label_dict)      # device tensors, no text file
        metrics = ev.evaluate()

    categories: the label map, a list of {"id", "name"} (read_labelmap); classes are id - 1, num_class is the largest id."""

    def __init__(self, categories, iou=0.5, device="cuda", exclusions=None):
        self.categories = list(categories)
        ids = [int(c["id"]) for c in self.categories]
        if not ids or min(ids) < 1:
            raise ValueError("classes should be 1-indexed")
        self.class_ids = set(ids)
        self.num_class = max(ids)
        self.iou = iou
        self.device = torch.device(device)
        self.excluded = set(exclusions) if exclusions else set()
        self._gt = {}                                  # image key -> (boxes [m,4] f64 xyxy, classes [m] int32), input order
        self._det_keys = {}                            # image key -> image number, in the order the detections were added
        self._det_rows = []                            # rows per image
        self._chunks = []                              # (boxes [n,4] f64, scores [n] f64, classes [n] int32, image [n] int64) on the device
        self._status = None
        self._luts = {}
        self._cache = None

    # ---- ground truth ----------------------------------------------------------------------------------------------------------------
    def add_groundtruth(self, image_key, boxes_xyxy, label_ids):
        """The ground truth of one image: boxes [m,4] (x1,y1,x2,y2) and their label ids.  Ids outside the label map are dropped; a key
        of the exclusion set is ignored, also when the exclusion arrives later (evaluate() looks at the set as it then stands); a key
        added twice raises (as object_detection_evaluation.py:175-176 does)."""
        if image_key in self.excluded:
            return
        if image_key in self._gt:
            raise ValueError("ground truth of image %s was added before" % image_key)
        boxes = np.asarray(boxes_xyxy, np.float64).reshape(-1, 4)
        ids = np.asarray(label_ids, np.int64).reshape(-1)
        if len(boxes) != len(ids):
            raise ValueError("boxes and label ids differ in length")
        keep = np.asarray([int(v) in self.class_ids for v in ids], bool)
        boxes, ids = boxes[keep], ids[keep]
        if not bool(np.all((boxes[:, 0] < boxes[:, 2]) & (boxes[:, 1] < boxes[:, 3]))):
            raise ValueError("ground-truth boxes must have positive area (image %s)" % image_key)
        if len(ids) > GT_ROWS_MAX:
            raise ValueError("more than %d ground-truth rows in image %s" % (GT_ROWS_MAX, image_key))
        self._gt[image_key] = (boxes, (ids - 1).astype(np.int32))
        self._cache = None

    def add_groundtruth_csv(self, file, exclusions=None):
        """Ground truth from a CSV in the AVA format; `exclusions` (a set of image keys, or a file / path of `video,timestamp` rows) is
        added to the evaluator's exclusion set first."""
        self._exclude(exclusions)
        boxes, labels, _ = read_ava_csv(file, self.class_ids)
        for key in boxes:
            self.add_groundtruth(key, boxes[key], labels[key])

    def _exclude(self, exclusions):
        if exclusions is None:
            return
        self._cache = None
        if isinstance(exclusions, (set, frozenset, list, tuple)):
            self.excluded |= set(exclusions)
        else:
            self.excluded |= read_exclusions(exclusions)

    # ---- detections ------------------------------------------------------------------------------------------------------------------
    def _new_image(self, key, rows):
        if key in self.excluded:
            return -1
        if key in self._det_keys:
            warnings.warn("detections of image %s have already been added; these are ignored" % key)      # (as :588-592 does)
            return -1
        self._det_keys[key] = len(self._det_rows)
        self._det_rows.append(int(rows))
        return self._det_keys[key]

    def _lut(self, label_dict):
        """class index of postprocess() -> class of the evaluator (label id - 1), -1 where the id is not in the label map; one extra
        entry (-1) at the end that indices outside the table are sent to"""
        sig = None if label_dict is None else tuple(sorted((int(k), int(v)) for k, v in label_dict.items()))
        if sig not in self._luts:
            pairs = [(c, c + 1) for c in range(self.num_class)] if sig is None else list(sig)
            n = max([c for c, _ in pairs] + [0]) + 1
            lut = np.full(n + 1, -1, np.int32)
            for c, lab in pairs:
                if c >= 0 and lab in self.class_ids:
                    lut[c] = lab - 1
            self._luts[sig] = torch.from_numpy(lut).to(self.device)
        return self._luts[sig]

    def add_detections(self, dets, infos, label_dict=None):
        """One iteration of driver.postprocess()'s result: per clip {boxes [m,4] fp32 normalised, scores [m], labels [m] (class index)}
        on the device, `infos` per clip {'video_name', 'fid'} and label_dict (class index -> label id; index + 1 when None) as for
        driver.detections_csv.  Boxes and scores are rounded to the four significant digits of that text on the device
        (step_round_sig4), so the result is what the reference computes from the file detections_csv would have written."""
        boxes, scores, labels, image = [], [], [], []
        for d, info in zip(dets, infos):
            n = int(d["scores"].shape[0])
            k = self._new_image(image_key(info["video_name"], info["fid"]), n)
            if k < 0 or n == 0:
                continue
            boxes.append(d["boxes"].reshape(-1, 4).float())
            scores.append(d["scores"].reshape(-1).float())
            labels.append(d["labels"].reshape(-1).long())
            image.append(np.full(n, k, np.int64))
        self._cache = None
        if not boxes:
            return
        dev = self.device
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        n = sum(len(v) for v in image)
        flat = torch.cat([torch.cat(boxes).to(dev).reshape(-1), torch.cat(scores).to(dev)])
        r = ops.round_sig4(flat, self._status)
        lut = self._lut(label_dict)
        lab = torch.cat(labels).to(dev)
        last = lut.numel() - 1
        lab = lab.masked_fill((lab < 0) | (lab > last), last)
        self._chunks.append((r[:4 * n].view(n, 4), r[4 * n:], lut[lab], torch.from_numpy(np.concatenate(image)).to(dev)))

    def add_detections_csv(self, file, exclusions=None):
        """Detections from a CSV that already exists (`video,timestamp,x1,y1,x2,y2,action_id,score`), parsed on the host as the
        reference parses it."""
        self._exclude(exclusions)
        boxes, labels, scores = read_ava_csv(file, self.class_ids)
        bx, sc, cl, im = [], [], [], []
        for key in boxes:
            k = self._new_image(key, len(boxes[key]))
            if k < 0:
                continue
            bx.append(np.asarray(boxes[key], np.float64).reshape(-1, 4))
            sc.append(np.asarray(scores[key], np.float64))
            cl.append(np.asarray(labels[key], np.int32) - 1)
            im.append(np.full(len(boxes[key]), k, np.int64))
        self._cache = None
        if not bx:
            return
        dev = self.device
        self._chunks.append(tuple(torch.from_numpy(np.concatenate(v)).to(dev) for v in (bx, sc, cl, im)))

    # ---- evaluation ------------------------------------------------------------------------------------------------------------------
    def _prepare(self):
        """what the host knows, uploaded once per state: the detection rows as one list, the ground truth of the images that have
        detections in their order, ground-truth rows per class"""
        if self._cache is not None:
            return self._cache
        dev, NC, NI = self.device, self.num_class, len(self._det_rows)
        num_gt = np.zeros(NC, np.int64)
        gt = {key: v for key, v in self._gt.items() if key not in self.excluded}       # (a key may have been excluded after its ground truth came)
        for _, cls in gt.values():
            num_gt += np.bincount(cls, minlength=NC)
        gb, gc, gs = [np.zeros((0, 4), np.float64)], [np.zeros(0, np.int32)], np.zeros(NI + 1, np.int64)
        for key, k in self._det_keys.items():
            if key in gt:
                gb.append(gt[key][0])
                gc.append(gt[key][1])
                gs[k + 1] = len(gt[key][1])
        gt_max = int(gs.max()) if NI else 0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        c = {"NI": NI, "gt_max": gt_max, "num_gt_host": num_gt, "num_gt": up(num_gt), "gt_boxes": up(np.concatenate(gb)),
             "gt_cls": up(np.concatenate(gc)), "gt_start": up(np.cumsum(gs)), "rows_max": max(self._det_rows + [0])}
        if self._chunks:
            c["det"] = tuple(torch.cat([ch[j] for ch in self._chunks]) for j in range(4))
            gone = np.asarray([key in self.excluded for key in self._det_keys], bool)
            if gone.any():                                             # a key excluded after its detections came: its rows leave every class
                boxes, score, cls, img = c["det"]
                c["det"] = (boxes, score, cls.masked_fill(up(gone)[img], -1), img)
            c["R"] = int(c["det"][1].numel())
        else:
            c["R"] = 0
        c["ar_img"] = torch.arange(NI + 1, device=dev)
        c["ar_cls"] = torch.arange(NC + 1, device=dev)
        self._cache = c
        return c

    def _labelling_order(self, c):
        """two stable sorts: image ascending, score descending, among equal scores the later row first -> (order [R], det_start [NI+1])"""
        _, score, _, img = c["det"]
        o = torch.flip(torch.sort(score, stable=True).indices, dims=(0,))
        o = o[torch.sort(img[o], stable=True).indices]
        return o, torch.searchsorted(img[o], c["ar_img"])

    def _class_order(self, c, label, cls_a, score_a):
        """two stable sorts on the rows in labelling order: class ascending, score descending, among equal scores the later position of
        the class's list over the images first; removed rows and rows outside the label map go behind the last class
        -> (key [R], order [R], cls_start [NC+1])"""
        NC = self.num_class
        key = cls_a.long().masked_fill((label == 2) | (cls_a < 0), NC)
        p = torch.flip(torch.sort(score_a, stable=True).indices, dims=(0,))
        p = p[torch.sort(key[p], stable=True).indices]
        return key, p, torch.searchsorted(key[p], c["ar_cls"])

    def evaluate(self, full=False):
        """-> the reference's dict: 'PascalBoxes_Precision/mAP@0.5IOU' and 'PascalBoxes_PerformanceByCategory/AP@0.5IOU/<name>' for every
        id of the label map (Python floats, NaN for a class without ground truth).  full=True: (dict, details) with details = {"ap" [NC],
        "num_gt" [NC], and per class (lists of NC numpy arrays, score-descending) "scores", "labels", "precision", "recall"}."""
        c = self._prepare()
        dev, NC, NI, R = self.device, self.num_class, c["NI"], c["R"]
        flags = [torch.zeros(1, dtype=torch.float64, device=dev) if self._status is None else self._status.double()]
        if R:
            o, det_start = self._labelling_order(c)
            boxes, score, cls, img = c["det"]
            cls_a, score_a = cls[o], score[o]
            label, match = ops.eval_match(boxes[o], cls_a, det_start, c["gt_boxes"], c["gt_cls"], c["gt_start"], c["gt_max"], self.iou)
            key, p, cls_start = self._class_order(c, label, cls_a, score_a)
            label_b, score_b = label[p], score_a[p]
            flags.append((score <= SCORE_MIN).any().double().view(1))
            if c["rows_max"] > DETS_PER_CLASS_MAX:                      # (only then can one class of one image hold that many)
                ks = torch.sort(img[o] * (NC + 1) + key).values
                run = torch.arange(R, device=dev) - torch.searchsorted(ks, ks)
                flags.append(((run >= DETS_PER_CLASS_MAX) & (ks % (NC + 1) < NC)).any().double().view(1))
        else:
            cls_start = torch.zeros(NC + 1, dtype=torch.int64, device=dev)
            label_b = torch.zeros(0, dtype=torch.uint8, device=dev)
            score_b = torch.zeros(0, dtype=torch.float64, device=dev)
        precision, recall, ap = ops.eval_ap(cls_start, label_b, c["num_gt"])
        host = torch.cat([ap] + flags).cpu().tolist()                   # the one host synchronisation
        ap, flags = host[:NC], host[NC:]
        if flags[0]:
            raise ValueError("add_detections: a box coordinate or score outside [1e-9, 1e4) in magnitude, inf or NaN")
        if len(flags) > 1 and flags[1]:
            raise ValueError("a detection score <= %g (the reference would drop the row)" % SCORE_MIN)
        if len(flags) > 2 and flags[2]:
            raise ValueError("more than %d detections of one class in one image (the reference would cut the list)" % DETS_PER_CLASS_MAX)
        have = [v for v in ap if not math.isnan(v)]
        mean = float("nan")
        if have:
            mean = 0.0
            for v in have:                                              # class order
                mean += v
            mean /= len(have)
        metrics = {"PascalBoxes_Precision/mAP@{}IOU".format(self.iou): mean}
        names = {int(cat["id"]): cat["name"] for cat in self.categories}
        for idx in range(NC):
            if idx + 1 in names:
                metrics["PascalBoxes_PerformanceByCategory/AP@{}IOU/{}".format(self.iou, names[idx + 1])] = ap[idx]
        if not full:
            return metrics
        cs = cls_start.cpu().tolist()
        parts = [t.cpu().numpy() for t in (score_b, label_b, precision, recall)]
        details = {"ap": np.asarray(ap, np.float64), "num_gt": c["num_gt_host"].copy()}
        for name, arr in zip(("scores", "labels", "precision", "recall"), parts):
            details[name] = [arr[cs[k]:cs[k + 1]].copy() for k in range(NC)]
        return metrics, details


def ava_evaluation(root, result_file, gt_file=None, iou=0.5, device="cuda"):
    """utils/eval_utils.py:12-23 with its signature and file names: the label map, the exclusions and (by default) the ground truth are
    read from `root`, the detections from result_file; returns the reference's dict of metrics.  Like the reference's, the evaluation runs
    at IoU 0.5 whatever `iou` says (the reference never passes it on).  Bind it in place of the reference's function."""
    files = {what: root + name for what, name in AVA_FILES.items()}
    categories, _ = read_labelmap(files["labelmap"])
    ev = FrameMAP(categories, iou=0.5, device=device, exclusions=read_exclusions(files["exclusions"]))
    ev.add_groundtruth_csv(files["groundtruth"] if gt_file is None else gt_file)
    ev.add_detections_csv(result_file)
    return ev.evaluate()
