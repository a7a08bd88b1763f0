"""The fused detection tail for clips of more than 64 tubes on the real gfx950 library: the cases of tests/detect_cases.py (shared with
the interpreter run of tests/test_emul_detect.py) plus what only exists on the device -- the count of host synchronisations of
postprocess / postprocess_merged with and without the workgroup form, and postprocess behind a hipGraph replay of the C3 pipeline on
the 84 tubes per clip of --anchor_mode 3."""
import pytest
import torch

from tests import detect_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", DC.KERNEL_CASES)
def test_gpu_detect_kernel(name, bk, golden):
    getattr(DC, name)(bk, golden)


@pytest.mark.parametrize("name", DC.MODULE_CASES)
def test_gpu_detect_module(name, golden):
    getattr(DC, name)("cuda", golden)


def test_block_path_makes_one_host_synchronisation(golden):
    """torch.cuda.set_sync_debug_mode("warn") reports every synchronising call: on clips of 84 / 65 / 0 / 109 tubes a warmed postprocess and
    a warmed postprocess_merged each make exactly ONE (the copy of the row counts); with DETECT_BLOCK = False -- the general path -- they
    make more, which shows that the count measures the routing."""
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
    hist, nums = DC.golden_history(golden("detect_block_golden"), "cuda")
    args = DC._args(conf_thresh=0.4, evaluate_topk=-1, topk=-1)
    for on in (True, False):
        with DC.detect_block(on):
            for _ in range(2):                                                                    # (the per-layout constants are uploaded once)
                postprocess(args, hist)
                postprocess_merged(args, hist, global_thresh=0.8)
            a, b = reports(lambda: postprocess(args, hist)), reports(lambda: postprocess_merged(args, hist, global_thresh=0.8))
        print("DETECT_BLOCK %s: synchronising calls reported: postprocess %d, postprocess_merged %d" % (on, len(a), len(b)))
        if on:
            assert len(a) == 1 and len(b) == 1, (a, b)
        else:
            assert len(a) > 1 and len(b) > 1, (a, b)


def test_postprocess_behind_a_graph_replay_at_anchor_mode_3():
    """C3 at one clip of the 84 tubes of --anchor_mode 3 (bf16), captured: postprocess on the replay's history == _postprocess_general on
    it, iteration by iteration; a second replay gives the first one's rows."""
    from step_amd import driver, workloads

    dev = torch.device("cuda:0")
    w = workloads.C3Inference(dev, torch.bfloat16, batch=1, anchor_mode="3", graph=True)
    assert [int(t.shape[0]) for t in w.tubes] == [84]
    with torch.no_grad():
        hist = w.launch()
        res = driver.postprocess(w.args, hist)
        assert len(res) == 3 and sum(int(d["scores"].numel()) for clips in res for d in clips) > 0
        for it, clips in enumerate(res):
            gen = driver._postprocess_general(hist[it], [84], 0.01, 0.4, -1, -1, 400.0, 400.0)    # (postprocess' defaults)
            for a_, b_ in zip(gen, clips):
                assert all(torch.equal(a_[k], b_[k]) for k in DC.ROW_KEYS), it
        kept = [[{k: d[k].clone() for k in DC.ROW_KEYS} for d in clips] for clips in res]
        again = driver.postprocess(w.args, w.launch())
        for ca, cb in zip(kept, again):
            for a_, b_ in zip(ca, cb):
                assert all(torch.equal(a_[k], b_[k]) for k in DC.ROW_KEYS)
