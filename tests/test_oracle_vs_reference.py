"""The C restatement against the reference's OWN compiled C++ on seeded random inputs, bit for bit.

What the reference's operators returned on these inputs is stored in tests/golden/ref_ops_golden.npz (recorded from
oracle/_ref/_C.so by `python -m oracle.make_golden ref_ops`), so the comparisons run from a clean checkout.  Where the
reference build is present (`make -C oracle ref`), every stored output is also checked against a live call of it.
CPU only."""
import functools

import numpy as np
import pytest
import torch

import oracle

_refC = oracle.load_reference_C() if oracle.have_reference_C() else None
needs_refC = pytest.mark.skipif(_refC is None, reason="oracle/_ref/_C.so not built")


def roi_align_cases(seed):
    """(key, x, rois, (ph, pw), sampling_ratio) for one seed."""
    rs = np.random.RandomState(seed)
    B, C, H, W = rs.randint(1, 4), rs.randint(1, 9), rs.randint(5, 30), rs.randint(5, 30)
    x = rs.randn(B, C, H, W).astype(np.float32)
    K = rs.randint(1, 20)
    xy = rs.uniform(-40, 16 * max(H, W), (K, 2))
    wh = rs.uniform(-10, 16 * max(H, W), (K, 2))
    rois = np.concatenate([rs.randint(0, B, (K, 1)), xy, xy + wh], 1).astype(np.float32)
    ph, pw = rs.randint(1, 9), rs.randint(1, 9)
    return [("roi_align_s%d_sr%d" % (seed, sr), x, rois, (ph, pw), sr) for sr in (0, 1, 3)]


def nms_cases(seed):
    """(key, boxes, scores, thr) for one seed, fp32."""
    rs = np.random.RandomState(100 + seed)
    n = int(rs.choice([1, 2, 11, 34, 63, 64, 65, 300]))
    xy = rs.uniform(0, 300, (n, 2))
    wh = rs.uniform(1, 150, (n, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    scores = (rs.permutation(n) / n).astype(np.float32)
    return [("nms_s%d_t%d" % (seed, i), boxes, scores, thr) for i, thr in enumerate((0.0, 0.3, 0.4, 0.9))]


def nms_nan_cases():
    rs = np.random.RandomState(7)
    out = []
    for n in (12, 34, 80):
        xy = rs.uniform(0, 200, (n, 2))
        boxes = np.concatenate([xy, xy + rs.uniform(20, 150, (n, 2))], 1).astype(np.float32)
        scores = (rs.permutation(n) / n).astype(np.float32)
        scores[[3, n // 2]] = np.nan                                 # two NaNs that each overlap other boxes
        out.append(("nms_nan_n%d" % n, boxes, scores, 0.3))
    return out


def nms_f64_cases(seed):
    rs = np.random.RandomState(100 + seed)
    out = []
    for n in (1, 11, 34, 200):
        xy = rs.uniform(0, 300, (n, 2))
        boxes = np.concatenate([xy, xy + rs.uniform(5, 150, (n, 2))], 1)
        scores = rs.permutation(n).astype(np.float64) / n
        out += [("nms64_s%d_n%d_t%d" % (seed, n, i), boxes, scores, thr) for i, thr in enumerate((0.3, 0.4, 0.7))]
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """key -> a call of the reference operator (refC -> ndarray): what oracle.make_golden records."""
    calls = {}
    for seed in range(6):
        for key, x, rois, (ph, pw), sr in roi_align_cases(seed):
            calls[key] = lambda refC, x=x, rois=rois, ph=ph, pw=pw, sr=sr: refC.roi_align_forward(
                torch.from_numpy(x), torch.from_numpy(rois), 1 / 16., ph, pw, sr).numpy()
    for key, boxes, scores, thr in ([c for s in range(8) for c in nms_cases(s)] + nms_nan_cases() + [c for s in (0, 1) for c in nms_f64_cases(s)]):
        calls[key] = lambda refC, b=boxes, s=scores, t=thr: refC.nms(torch.from_numpy(b), torch.from_numpy(s), t).numpy()
    return calls


def reference(golden, key):
    """What the reference returned for `key`: the stored vector, checked against the live build where there is one."""
    g = golden("ref_ops_golden")[key]
    if _refC is not None:
        assert np.array_equal(all_cases()[key](_refC), g), "tests/golden/ref_ops_golden.npz no longer matches oracle/_ref/_C.so: " + key
    return g


@needs_refC
def test_exports():
    for name in ("nms", "roi_align_forward", "roi_align_backward", "roi_pool_forward", "roi_pool_backward"):
        assert hasattr(_refC, name)          # csrc/vision.cpp:30-36


@pytest.mark.parametrize("seed", range(6))
def test_roi_align_forward_random(golden, seed):
    for key, x, rois, pooled, sr in roi_align_cases(seed):
        out = oracle.roi_align_forward(x, rois, pooled, 1 / 16., sr)
        assert np.array_equal(out, reference(golden, key))


@pytest.mark.parametrize("seed", range(8))
def test_nms_random(golden, seed):
    for key, boxes, scores, thr in nms_cases(seed):
        assert np.array_equal(oracle.nms(boxes, scores, thr), reference(golden, key))


def test_nms_nan_scores_sort_first(golden):
    """NaN scores: torch's descending sort (nms_cpu.cpp:48) ranks them first; the restatement follows."""
    for key, boxes, scores, thr in nms_nan_cases():
        ref = reference(golden, key)
        assert len(ref) < len(scores)
        assert np.array_equal(oracle.nms(boxes, scores, thr), ref)


@needs_refC
def test_reference_has_no_cpu_backward_or_roipool():
    # csrc/ROIAlign.h:68, csrc/ROIPool.h:47,68 -- this is why those oracles are pinned indirectly
    x = torch.zeros(1, 1, 4, 4)
    r = torch.tensor([[0., 0, 0, 3, 3]])
    with pytest.raises(RuntimeError):
        _refC.roi_pool_forward(x, r, 1.0, 2, 2)
    with pytest.raises(RuntimeError):
        _refC.roi_align_backward(torch.zeros(1, 1, 2, 2), r, 1.0, 2, 2, 1, 1, 4, 4, 0)


@pytest.mark.parametrize("seed", [0, 1])
def test_nms_fp64_restatement_matches_the_reference_double_kernel(golden, seed):
    """AT_DISPATCH_FLOATING_TYPES (cpu/nms_cpu.cpp:95): double boxes run nms_cpu_kernel<double>; oracle.nms_f64 is bit-identical."""
    for key, boxes, scores, thr in nms_f64_cases(seed):
        assert np.array_equal(oracle.nms_f64(boxes, scores, thr), reference(golden, key))
