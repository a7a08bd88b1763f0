"""The frame-mAP evaluation on the real gfx950 library: the cases of tests/eval_cases.py (shared with the interpreter run of
tests/test_emul_eval.py) plus what only exists on the device -- the rounding of step_round_sig4 against the text round trip on the rows
a real C3 pipeline produces, and the count of evaluate()'s host synchronisations."""
import io

import numpy as np
import pytest
import torch

from tests import eval_cases as EV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", EV.KERNEL_CASES)
def test_gpu_eval_kernel(name, bk, golden):
    getattr(EV, name)(bk, golden)


@pytest.mark.parametrize("name", EV.MODULE_CASES)
def test_gpu_eval_module(name, golden):
    getattr(EV, name)("cuda", golden)


def test_frame_map_on_the_rows_of_a_c3_pipeline():
    """C3 at 4 clips x 34 tubes (bf16) -> postprocess -> FrameMAP.add_detections (fp32 rows rounded on the device) against ground truth
    made from some of its own top rows (jittered) == the numpy restatement fed the PARSED LINES of detections_csv for the same rows:
    the (score, label) list of every class exactly -- the device rounding equals the file round trip on real rows -- and AP within the
    bound.  Both iterations' worth of rows are used: the last two refinement iterations as eight images."""
    from step_amd import workloads
    from step_amd.driver import detections_csv, postprocess
    from step_amd.evaluate import FrameMAP, read_ava_csv

    dev = torch.device("cuda:0")
    w = workloads.C3Inference(dev, torch.bfloat16, batch=4, tubes=34, graph=True)
    with torch.no_grad():
        res = postprocess(w.args, w.launch(), conf_thresh=0.05)
    cats = [{"id": i, "name": "action %d" % i} for i in range(1, 61)]
    ev = FrameMAP(cats, device="cuda")
    text, parts = [], []
    for it in (len(res) - 2, len(res) - 1):
        infos = [{"video_name": "it%d" % it, "fid": 900 + b} for b in range(len(res[it]))]
        text += detections_csv(res[it], infos)
        parts.append((res[it], infos))
    boxes, labels, scores = read_ava_csv(io.StringIO("".join(text)), set(range(1, 61)))
    n_rows = sum(len(v) for v in scores.values())
    assert n_rows == len(text) and n_rows > 100, n_rows
    rs = np.random.RandomState(7)
    gt = {}
    for key in boxes:                                                             # ground truth: the image's top rows, jittered (some far enough to miss)
        b, l, s = np.asarray(boxes[key]), np.asarray(labels[key]), np.asarray(scores[key])
        top = np.argsort(s, kind="stable")[::-1][:12]
        gb = np.round(b[top] + rs.choice([0.004, 0.03, 0.12], (len(top), 1)) * rs.uniform(-1, 1, (len(top), 4)), 3)
        ok = (gb[:, 0] < gb[:, 2]) & (gb[:, 1] < gb[:, 3])
        gt[key] = (gb[ok], l[top][ok].astype(np.int32) - 1)
        ev.add_groundtruth(key, gb[ok], l[top][ok])
    for dets, infos in parts:
        ev.add_detections(dets, infos)
    metrics, full = ev.evaluate(full=True)
    rows = dict(num_class=60, gt=gt, images=[dict(key=k, box=np.asarray(boxes[k], np.float64), score=np.asarray(scores[k], np.float64),
                                                  cls=np.asarray(labels[k], np.int32) - 1) for k in boxes])
    want = EV.np_evaluate(rows)
    tp = sum(int(l.sum()) for l in want["labels"])
    ties = sum(len(s) - len(np.unique(s)) for s in want["scores"])
    print("rows %d, images %d, ground-truth rows %d, true positives %d, tied rows inside a class %d" % (n_rows, len(boxes), int(want["num_gt"].sum()), tp, ties))
    assert tp > 0
    for k in range(60):
        assert np.array_equal(full["scores"][k], want["scores"][k]) and np.array_equal(full["labels"][k], want["labels"][k]), k
    assert np.array_equal(full["num_gt"], want["num_gt"])
    per, bm = EV.ap_bounds(want["labels"], 60)
    assert np.array_equal(np.isnan(full["ap"]), np.isnan(want["ap"]))
    assert np.all(np.abs(np.nan_to_num(full["ap"] - want["ap"])) <= per) and abs(metrics["PascalBoxes_Precision/mAP@0.5IOU"] - want["map"]) <= bm


def test_evaluate_makes_one_host_synchronisation(golden):
    """torch.cuda.set_sync_debug_mode("warn") reports every synchronising call: a warmed evaluate() makes exactly ONE (the copy of the
    per-class AP with the status flags), on detections added as device tensors and on detections read from text."""
    import warnings

    def reports(fn):
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        return [str(x.message) for x in w if "synchronizing" in str(x.message) and "prototype" not in str(x.message)]

    x = torch.ones(8, device="cuda")
    assert len(reports(lambda: x.sum().item())) == 1 and len(reports(lambda: x + 1)) == 0        # the mode does report on this build
    c = EV.load_case(golden("eval_golden"), "A")
    for tag, ev in (("rows", EV.frame_map_rows(c, "cuda")), ("csv", EV.frame_map_csv(c, "cuda"))):
        for _ in range(2):                                                                        # (what the host knows is uploaded once per state)
            first = ev.evaluate()
        r = reports(ev.evaluate)
        print(tag, "synchronising calls reported for evaluate():", len(r))
        assert len(r) == 1, (tag, r)
        assert repr(ev.evaluate()) == repr(first)
