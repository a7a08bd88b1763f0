"""The cross-class merge of detections on the real gfx950 library: the cases of tests/merge_cases.py (shared with the interpreter run
of tests/test_emul_merge.py) plus what only exists on the device -- postprocess_merged behind a hipGraph replay of the C3 pipeline and the count of its host
synchronisations."""
import pytest
import torch

from tests import merge_cases as MG

pytestmark = pytest.mark.gpu

KEYS = ("boxes", "cluster", "labels", "scores", "tubes")


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", MG.KERNEL_CASES)
def test_gpu_merge_kernel(name, bk, golden):
    getattr(MG, name)(bk, golden)


@pytest.mark.parametrize("name", MG.MODULE_CASES)
def test_gpu_merge_module(name, golden):
    getattr(MG, name)("cuda", golden)


def test_postprocess_merged_behind_a_graph_replay():
    """C3 at 4 clips x 34 tubes (bf16), conf_thresh 0.4, top-k 300: postprocess_merged on the history a GraphedInference replay leaves in
    its static buffers == postprocess_merged on the eagerly computed history, result for result (whether the two histories are bit-equal
    is printed first), and on a copy of those buffers; both are held, exactly, to the host restatement of the merge on the rows
    postprocess() returns for the same history.  A second replay + merge gives the first one's result again."""
    from step_amd import workloads
    from step_amd.driver import inference, postprocess, postprocess_merged

    dev = torch.device("cuda:0")
    w = workloads.C3Inference(dev, torch.bfloat16, batch=4, tubes=34, graph=True)
    kw = dict(conf_thresh=0.4, evaluate_topk=1, topk=300)
    with torch.no_grad():
        hist_g = w.launch()
        res_g = postprocess_merged(w.args, hist_g, global_thresh=0.8, **kw)
        MG.check_against_rows(res_g, postprocess(w.args, hist_g, **kw), 0.8, "graph")
        rows = sum(int(d["scores"].numel()) for clips in res_g for d in clips)
        clusters = sum(int(d["boxes"].shape[0]) for clips in res_g for d in clips)
        assert len(res_g) == 3 and all(len(c) == 4 for c in res_g) and rows > 0 and 0 < clusters <= rows
        kept = [[{k: d[k].clone() for k in KEYS} for d in clips] for clips in res_g]
        cf = w.base(w.x)
        hist_e, _ = inference(w.args, cf, w.ctx(cf), w.nets, 3, w.tubes)
        res_e = postprocess_merged(w.args, hist_e, global_thresh=0.8, **kw)
        MG.check_against_rows(res_e, postprocess(w.args, hist_e, **kw), 0.8, "eager")
        same = all(torch.equal(a[k], b[k]) for a, b in zip(hist_g, hist_e) for k in ("pred_prob", "pred_loc"))
        print("graph replay vs eager history bit-equal: %s; rows %d, clusters %d" % (same, rows, clusters))
        for ca, cb in zip(res_g, res_e):
            for a, b in zip(ca, cb):
                assert all(torch.equal(a[k], b[k]) for k in KEYS)
        # ... and on a copy of the replay's static buffers
        hist_c = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in h.items()} for h in hist_g]
        for ca, cb in zip(res_g, postprocess_merged(w.args, hist_c, global_thresh=0.8, **kw)):
            for a, b in zip(ca, cb):
                assert all(torch.equal(a[k], b[k]) for k in KEYS)
        again = postprocess_merged(w.args, w.launch(), global_thresh=0.8, **kw)
        for ca, cb in zip(kept, again):
            for a, b in zip(ca, cb):
                assert all(torch.equal(a[k], b[k]) for k in KEYS)


def test_postprocess_merged_makes_one_host_synchronisation(golden):
    """torch.cuda.set_sync_debug_mode("warn") reports every synchronising call: on the <= 64 tubes path a warmed postprocess_merged makes
    exactly ONE (the copy of selected rows and clusters per group behind the step_detect_merge launch, driver._merge_segments), as many
    as postprocess() makes for the same history -- with and without top-k."""
    import warnings

    from step_amd.driver import postprocess, postprocess_merged

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
    g = golden("merge_golden")
    hist, nums = MG.fixture_history(g, "A", "cuda")
    for tag in ("all08", "top08"):
        conf, thr, etopk, topk = MG.case_cfg(g, tag)
        args = MG._args(conf_thresh=conf, evaluate_topk=etopk, topk=topk)
        for _ in range(2):                                                                        # (the per-layout constants are uploaded once)
            postprocess(args, hist)
            postprocess_merged(args, hist, global_thresh=thr)
        a, b = reports(lambda: postprocess(args, hist)), reports(lambda: postprocess_merged(args, hist, global_thresh=thr))
        print(tag, "synchronising calls reported: postprocess %d, postprocess_merged %d" % (len(a), len(b)))
        assert len(b) == 1 and len(a) == 1, (tag, a, b)
