"""Cases for gradient-norm clipping and the learning-rate schedules on the device (step_grad_norm_flat, step_grad_clip_flat,
step_lr_schedule; _FlatOptimizer.clip_grad_norm_ / step(max_grad_norm=), DeviceWarmupCosineLR / DeviceWarmupStepLR), driven on the host
interpreter by tests/test_emul_clip.py and on the real library by tests/test_gpu_clip.py.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda").

References.  Norms: a float64 numpy restatement, sqrt(sum(g.astype(f64)**2)) * grad_scale / scale rounded once to fp32, within ONE fp32
ulp -- derived, not measured: the fp64 sum of <= 2^17 exact squares carries a relative error below 2^-36 whatever its order, so only a
rounding boundary of the fp32 result that the two sums straddle can move it, and then by one ulp.  Schedules: the learning rates the
reference's own WarmupCosineLR / WarmupStepLR left in param_groups (tests/golden/lr_schedule_golden.json, tools/make_lr_golden.py), within
one fp32 ulp of f32(recorded) -- the device's double-precision cos / pow and its contraction of multiply-adds against CPython's libm; the
rounding to fp32 absorbs all but boundary cases.  Optimizers: torch.optim preceded by torch.nn.utils.clip_grad_norm_."""
import ctypes
import hashlib
import json
import os

import numpy as np
import torch

import step_amd
from tests import sgd_cases as SC

f32, f64 = np.float32, np.float64
SIZES, N = SC.SIZES, SC.N                                    # the project's six-segment arena
LONG_SIZES = [64, 70000, 61008]                              # one segment over many chunks, a chunk boundary inside a segment, the grid wraps
LONG_N = sum(LONG_SIZES)
assert LONG_N == 131072

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule_golden.json")
_cache = {}


def lr_golden():
    if "lr" not in _cache:
        with open(_GOLDEN) as f:
            _cache["lr"] = json.load(f)
    return _cache["lr"]


def arena(which):
    """(sizes, gradient) of the small / long arena; computed once, handed out as copies"""
    if which not in _cache:
        if which == "small":
            _cache[which] = (SIZES, SC._grad(np.random.RandomState(21)))
        else:
            _cache[which] = (LONG_SIZES, SC._grad(np.random.RandomState(22), LONG_N))
    sizes, g = _cache[which]
    return sizes, g.copy()


def ulps(a, b):
    """distance in fp32 ulps between two arrays of finite, non-negative floats"""
    a, b = np.atleast_1d(np.asarray(a, f32)), np.atleast_1d(np.asarray(b, f32))
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ref_norms(g, sizes, grad_scale=1.0, scale=1.0):
    """the float64 restatement: (total, per segment), each rounded once to fp32"""
    g64 = g.astype(f64)
    tot = f32(np.sqrt(np.sum(g64 ** 2)) * f64(grad_scale) / f64(scale))
    seg = np.array([np.sqrt(np.sum(c ** 2)) * f64(grad_scale) / f64(scale) for c in SC._split(g64, sizes)]).astype(f32)
    return tot, seg


def ref_coef(norm, max_norm):
    """torch's arithmetic in fp32, from the REPORTED norm"""
    return np.minimum(f32(1.0), f32(max_norm) / (f32(norm) + f32(1e-6)))


class Norm:
    """the buffers of one step_grad_norm_flat / step_grad_clip_flat call sequence on a backend"""

    def __init__(self, bk, sizes, g, amp=None):
        self.bk, self.sizes, self.n = bk, sizes, int(sum(sizes))
        self.G = bk.dev(g.copy())
        self.ends = bk.dev(np.cumsum(sizes).astype(np.int64))
        self.nbytes = int(bk.lib.step_grad_norm_workspace_bytes(self.n, len(sizes)))
        self.ws = bk.dev(np.full(max(self.nbytes // 8, 1), np.nan, f64))          # nothing in it needs initialising
        self.seg = bk.dev(np.full(len(sizes), -7.0, f32))
        self.stats = bk.dev(np.full(4, -7.0, f32))
        self.amp = None if amp is None else bk.dev(np.array(amp, f32))

    def norm(self, max_norm, grad_scale=1.0):
        return self.bk.lib.step_grad_norm_flat(self.G.ptr, self.n, self.ends.ptr, len(self.sizes), grad_scale, None if self.amp is None else self.amp.ptr,
                                               max_norm, self.ws.ptr, self.nbytes, self.seg.ptr, self.stats.ptr, self.bk.stream)

    def clip(self):
        return self.bk.lib.step_grad_clip_flat(self.G.ptr, self.n, self.stats.ptr, self.bk.stream)


# ---- kernel cases ------------------------------------------------------------------------------------------------------------
def _norm_case(bk, which, grad_scale):
    sizes, g = arena(which)
    x = Norm(bk, sizes, g)
    assert x.norm(1.0, grad_scale) == 0
    tot, seg = ref_norms(g, sizes, abs(f64(f32(grad_scale))))
    st = x.stats.get()
    print("grad_norm[%s] %s: total %.9g (restatement %.9g, %d ulp), worst segment %d ulp" % (which, bk.name, st[0], tot, int(ulps(st[0], tot)[0]),
                                                                                             int(ulps(x.seg.get(), seg).max())))
    assert ulps(st[0], tot)[0] <= 1 and np.all(ulps(x.seg.get(), seg) <= 1)
    assert st[2] == 0.0 and st[3] == 0.0
    assert np.array_equal(x.G.get(), g)                       # the norm pass only reads
    return x, g


def case_norm_small(bk, golden):
    """total_norm and every seg_norm of the six-segment arena within 1 fp32 ulp of the float64 restatement (grad_scale -0.25: its absolute
    value counts), and the cross-check against torch.nn.utils.clip_grad_norm_ on this arena only: the float64 restatement was measured
    against torch's fp32 norm on the CPU at 2.1e-7 relative worst case over 200 seeds, bounded here at 1e-6 (on the long arena torch's
    own fp32 accumulation is 5e-6 off, so it is no yardstick there)."""
    _norm_case(bk, "small", -0.25)
    sizes, g = arena("small")
    x = Norm(bk, sizes, g)
    assert x.norm(1.0, 1.0) == 0
    tp = [torch.nn.Parameter(torch.zeros(s)) for s in sizes]
    SC._set_grads(tp, g, sizes)
    want = float(torch.nn.utils.clip_grad_norm_(tp, 1e30))
    got = float(x.stats.get()[0])
    print("grad_norm[small] %s against torch: %.3e relative" % (bk.name, abs(got - want) / want))
    assert abs(got - want) <= 1e-6 * want


def case_norm_long(bk, golden):
    """the same on the long arena (131 072 elements in three segments, grad_scale float32(1/3)): a segment over many chunks, a chunk
    boundary inside a segment, more chunks than workgroups on the interpreter"""
    _norm_case(bk, "long", float(f32(1.0 / 3.0)))


def _clip_case(bk, which):
    sizes, g = arena(which)
    tot, _ = ref_norms(g, sizes)
    max_norm = float(f32(0.1) * tot)
    x = Norm(bk, sizes, g)
    assert x.norm(max_norm) == 0 and x.clip() == 0
    st = x.stats.get()
    coef = ref_coef(st[0], max_norm)
    assert st[1].tobytes() == f32(coef).tobytes() and 0.09 < coef < 0.11, (st, coef)
    assert np.array_equal(x.G.get(), (g * f32(coef)).astype(f32))       # one rounding per element
    # no clip: the coefficient is exactly 1.0 and not a byte of the arena changes
    y = Norm(bk, sizes, g)
    assert y.norm(float(f32(10.0) * tot)) == 0 and y.clip() == 0
    assert y.stats.get()[1].tobytes() == f32(1.0).tobytes() and y.stats.get()[2] == 0.0
    assert digest(y.G.get()) == digest(g)


def case_clip_small(bk, golden):
    """max_norm = 0.1 x the norm: stats[1] is min(1, f32(max_norm) / (stats[0] + f32(1e-6))) in numpy fp32 from the reported norm, bit for
    bit, and every element f32(g * coef), bit for bit; max_norm = 10 x the norm: coefficient exactly 1.0, the arena's digest unchanged."""
    _clip_case(bk, "small")


def case_clip_long(bk, golden):
    _clip_case(bk, "long")


case_clip_long.__doc__ = case_clip_small.__doc__


def case_zero_gradient(bk, golden):
    """a zero gradient: norm 0 (every segment too), coefficient 1, the arena stays zero"""
    sizes, _ = arena("small")
    x = Norm(bk, sizes, np.zeros(N, f32))
    assert x.norm(1.0) == 0 and x.clip() == 0
    assert np.array_equal(x.stats.get(), np.array([0.0, 1.0, 0.0, 0.0], f32)) and not x.seg.get().any() and not x.G.get().any()


def case_nonfinite(bk, golden):
    """One inf, then one NaN, at the first element, at the last element of the long segment and in the last chunk; and four elements of
    3e38 (finite, but the norm overflows fp32): nonfinite = 1, coefficient exactly 1, the gradient untouched (torch would multiply by 0 or
    NaN: the documented divergence that leaves the overflow to the loss scaler's skip).  Elements of 1e30 give a finite, correct norm --
    the reason for the fp64 accumulation."""
    sizes, g0 = arena("long")
    places = (0, LONG_SIZES[0] + LONG_SIZES[1] - 1, LONG_N - 5)
    for bad in (np.inf, np.nan):
        for at in places:
            g = g0.copy()
            g[at] = bad
            x = Norm(bk, sizes, g)
            assert x.norm(1e-3) == 0 and x.clip() == 0
            st = x.stats.get()
            assert st[2] == 1.0 and st[1].tobytes() == f32(1.0).tobytes() and not np.isfinite(st[0]), (bad, at, st)
            assert np.array_equal(x.G.get(), g, equal_nan=True), (bad, at)
    g = g0.copy()
    g[[3, 70001, 100000, LONG_N - 1]] = f32(3e38)
    x = Norm(bk, sizes, g)
    assert x.norm(1e-3) == 0 and x.clip() == 0
    st = x.stats.get()
    assert st[2] == 1.0 and st[1] == 1.0 and np.isinf(st[0]) and np.array_equal(x.G.get(), g), st
    g = g0.copy()
    g[[3, 70001, 100000, LONG_N - 1]] = f32(1e30)
    x = Norm(bk, sizes, g)
    assert x.norm(1.0) == 0
    tot, seg = ref_norms(g, sizes)
    st = x.stats.get()
    assert st[2] == 0.0 and np.isfinite(st[0]) and ulps(st[0], tot)[0] <= 1 and np.all(ulps(x.seg.get(), seg) <= 1), (st, tot)
    assert st[1].tobytes() == f32(ref_coef(st[0], 1.0)).tobytes()


def case_loss_scaling(bk, golden):
    """amp_state[0] = 1024: the norm of 1024 g equals the norm of g within 1 ulp (the clip works in UN-scaled units).  And an arena that
    holds an inf: norm + clip leave it alone, and the step_sgd_flat_amp that follows skips exactly as it does without the clip --
    parameters, buffer, gradient, counter and loss-scale state equal to a twin's that never saw the clip, bit for bit."""
    sizes, g = arena("small")
    tot, seg = ref_norms(g, sizes, 0.5)
    x = Norm(bk, sizes, (g * f32(1024.0)).astype(f32), amp=[1024.0, 3.0, 0.0, 0.0])
    assert x.norm(1.0, 0.5) == 0
    assert ulps(x.stats.get()[0], tot)[0] <= 1 and np.all(ulps(x.seg.get(), seg) <= 1)
    assert np.array_equal(x.amp.get(), np.array([1024.0, 3.0, 0.0, 0.0], f32))        # read only
    rs = np.random.RandomState(4)
    p0, b0 = rs.randn(N).astype(f32), rs.randn(N).astype(f32)
    gs = (g * f32(1024.0)).astype(f32)
    gs[700] = np.inf
    out = []
    for with_clip in (True, False):
        y = Norm(bk, sizes, gs, amp=[1024.0, 3.0, 0.0, 0.0])
        P, B, cnt = bk.dev(p0.copy()), bk.dev(b0.copy()), bk.dev(np.full(1, 2, np.int64))
        LR, WD = bk.dev(np.array(SC.LRS, f32)), bk.dev(np.array(SC.WDS, f32))
        if with_clip:
            assert y.norm(1e-3, 0.5) == 0 and y.clip() == 0
            assert y.stats.get()[2] == 1.0 and np.array_equal(y.G.get(), gs)
        assert bk.lib.step_sgd_flat_amp(P.ptr, y.G.ptr, B.ptr, N, y.ends.ptr, LR.ptr, WD.ptr, len(sizes), 0.9, 0.0, 0, cnt.ptr, 0.5, 0, y.amp.ptr,
                                        2.0, 0.5, 100, bk.stream) == 0
        out.append((P.get().copy(), B.get().copy(), y.G.get().copy(), cnt.get().copy(), y.amp.get().copy()))
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert np.array_equal(out[0][0], p0) and np.array_equal(out[0][1], b0) and int(out[0][3][0]) == 2          # skipped
    assert np.array_equal(out[0][4], np.array([512.0, 0.0, 0.0, 0.0], f32))


def case_determinism(bk, golden):
    """two runs on the same long arena: identical bits in stats, seg_norm and the clipped arena (fixed summation order, no atomics)"""
    sizes, g = arena("long")
    tot, _ = ref_norms(g, sizes)
    runs = []
    for _ in range(2):
        x = Norm(bk, sizes, g)
        assert x.norm(float(f32(0.1) * tot), 0.5) == 0 and x.clip() == 0
        runs.append((digest(x.stats.get()), digest(x.seg.get()), digest(x.G.get())))
    assert runs[0] == runs[1] and runs[0][2] != digest(g)


def case_clip_errors(bk, golden):
    """Every refusal of the three entry points with the outputs pre-filled and found unchanged; n == 0 is accepted.  A seg_end table whose
    last entry is not n lives in DEVICE memory and the call reads nothing back: it is refused on the device -- nothing is written -- and
    the status cannot say so (include/step_amd.h)."""
    sizes, g = arena("small")
    x = Norm(bk, sizes, g)
    L, s, ns = bk.lib, bk.stream, len(sizes)
    nan = float("nan")

    def norm(g_=x.G.ptr, n=N, ends=x.ends.ptr, nseg=ns, max_norm=1.0, ws=x.ws.ptr, nbytes=x.nbytes, stats=x.stats.ptr):
        return L.step_grad_norm_flat(g_, n, ends, nseg, 1.0, None, max_norm, ws, nbytes, x.seg.ptr, stats, s)

    assert norm(max_norm=0.0) < 0 and norm(max_norm=-1.0) < 0 and norm(max_norm=nan) < 0
    assert norm(n=N + 2) < 0 and norm(n=-4) < 0
    assert norm(g_=None) < 0 and norm(ends=None) < 0 and norm(ws=None) < 0 and norm(stats=None) < 0
    assert norm(nseg=0) < 0 and norm(nseg=4097) < 0 and norm(nseg=-1) < 0
    assert norm(nbytes=x.nbytes - 8) < 0
    assert norm(g_=SC._shift(x.G.ptr, 4)) < 0 and norm(ws=SC._shift(x.ws.ptr, 4)) < 0
    short = bk.dev((np.cumsum(sizes) - 4).astype(np.int64))                        # last entry n - 4
    assert norm(ends=short.ptr) == 0                                               # refused on the device: see the docstring
    assert L.step_grad_clip_flat(x.G.ptr, N + 2, x.stats.ptr, s) < 0 and L.step_grad_clip_flat(x.G.ptr, -4, x.stats.ptr, s) < 0
    assert L.step_grad_clip_flat(None, N, x.stats.ptr, s) < 0 and L.step_grad_clip_flat(x.G.ptr, N, None, s) < 0
    assert L.step_grad_clip_flat(SC._shift(x.G.ptr, 4), N, x.stats.ptr, s) < 0
    assert np.array_equal(x.G.get(), g) and np.all(x.stats.get() == f32(-7.0)) and np.all(x.seg.get() == f32(-7.0)) and np.isnan(x.ws.get()).all()
    assert norm(g_=None, n=0, ends=None, ws=None, nbytes=0) == 0 and L.step_grad_clip_flat(None, 0, x.stats.ptr, s) == 0       # n == 0: no launch
    assert np.all(x.stats.get() == f32(-7.0))
    assert L.step_grad_norm_workspace_bytes(N, ns) >= 8 * (1 + ns) and L.step_grad_norm_workspace_bytes(0, ns) == 8 * ns
    # the schedule
    it, base, lr = bk.dev(np.full(1, 5, np.int64)), bk.dev(np.array([1e-3, 2e-3], f64)), bk.dev(np.full(2, -7.0, f32))
    ms = bk.dev(np.array([10, 30, 60], np.int64))

    def sched(kind=0, i=it.ptr, b=base.ptr, o=lr.ptr, nseg=2, m=ms.ptr, nm=3, warm=10):
        return L.step_lr_schedule(kind, i, b, o, nseg, m, nm, warm, 0.1, 0.01, 0.5, s)

    assert sched(kind=2) < 0 and sched(kind=-1) < 0
    assert sched(i=None) < 0 and sched(b=None) < 0 and sched(o=None) < 0 and sched(m=None) < 0
    assert sched(nseg=0) < 0 and sched(nseg=4097) < 0
    assert sched(nm=65) < 0 and sched(nm=1) < 0 and sched(kind=1, nm=-1) < 0 and sched(warm=-1) < 0
    assert int(it.get()[0]) == 5 and np.all(lr.get() == f32(-7.0))
    assert sched(kind=1, m=None, nm=0) == 0 and int(it.get()[0]) == 6               # a step schedule without milestones: warm-up, then base
    assert np.all(ulps(lr.get(), (np.array([1e-3, 2e-3]) * (0.1 * (1 - 0.6) + 0.6)).astype(f32)) <= 1)


def case_lr_schedule(bk, golden):
    """step_lr_schedule against the recorded runs of the reference's schedulers: for every case and iteration seg_lr within 1 fp32 ulp of
    f32(recorded lr), on a six-segment table whose segments map onto the three base lrs; the counter reads 1, 2, 3, ... from 0 (and 0 from
    -1: what a scheduler's construction leaves); the resumed case, started at last_epoch 45, continues the recorded sequence."""
    gold = lr_golden()
    groups = [0, 1, 2, 2, 0, 1]
    base = np.array([gold["base_lrs"][k] for k in groups], f64)
    worst, total, equal = 0, 0, 0
    for case in gold["cases"]:
        a = case["args"]
        if case["kind"] == "cosine":
            kind, table, p0, p1 = 0, [a["warmup_iters"]] + a["milestones"], a["min_ratio"], a["cycle_decay"]
        else:
            kind, table, p0, p1 = 1, a["milestones"], a["gamma"], 1.0
        it, B, LR = bk.dev(np.full(1, case["last_epoch"], np.int64)), bk.dev(base.copy()), bk.dev(np.zeros(len(groups), f32))
        ms = bk.dev(np.array(table, np.int64))
        for k, rec in enumerate(case["lrs"]):
            assert bk.lib.step_lr_schedule(kind, it.ptr, B.ptr, LR.ptr, len(groups), ms.ptr, len(table), a["warmup_iters"], a["warmup_factor"], p0, p1,
                                           bk.stream) == 0
            assert int(it.get()[0]) == case["first_epoch"] + k
            want = np.array([rec[g] for g in groups]).astype(f32)
            d = ulps(LR.get(), want)
            worst, total, equal = max(worst, int(d.max())), total + d.size, equal + int((d == 0).sum())
            assert d.max() <= 1, (case["name"], k, LR.get(), want)
        assert case["first_epoch"] == case["last_epoch"] + 1
    print("lr_schedule %s: worst %d ulp, %d of %d bit-equal" % (bk.name, worst, equal, total))


def big_grad_norm_full_size(bk, golden):
    """The norm and the clip at the C4 parameter count (44.4 M fp32 in 11 segments: more chunks than workgroups, so the grid wraps on the
    device too) against torch's float64 norm on the same device, within 1 fp32 ulp (2^26 squares: the fp64 sum is good to 2^-27 relative
    in the worst case, still far inside half an fp32 ulp); clipped elements bit-equal to torch's fp32 multiply; two runs identical."""
    torch.manual_seed(5)
    sizes = [4_000_000 + 64 * i for i in range(11)]
    n = sum(sizes)
    G = torch.randn(n, device="cuda") * 3.0
    G0 = G.clone()
    ends = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device="cuda")
    nbytes = int(bk.lib.step_grad_norm_workspace_bytes(n, len(sizes)))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    seg, stats = torch.zeros(len(sizes), device="cuda"), torch.zeros(4, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    want = G0.double().square().sum().sqrt().float()
    want_seg = torch.stack([c.double().square().sum().sqrt() for c in torch.split(G0, sizes)]).float()
    got = []
    for _ in range(2):
        G.copy_(G0)
        assert bk.lib.step_grad_norm_flat(vp(G), n, vp(ends), len(sizes), 1.0, None, 100.0, vp(ws), nbytes, vp(seg), vp(stats), bk.stream) == 0
        assert bk.lib.step_grad_clip_flat(vp(G), n, vp(stats), bk.stream) == 0
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy().copy(), seg.cpu().numpy().copy(), G.clone()))
    st = got[0][0]
    assert ulps(st[0], want.cpu().numpy())[0] <= 1 and np.all(ulps(got[0][1], want_seg.cpu().numpy()) <= 1), (st, float(want))
    assert st[1].tobytes() == f32(ref_coef(st[0], 100.0)).tobytes() and st[1] < 1.0 and st[2] == 0.0
    assert torch.equal(got[0][2], G0 * float(st[1]))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])


KERNEL_CASES = ["case_norm_small", "case_norm_long", "case_clip_small", "case_clip_long", "case_zero_gradient", "case_nonfinite",
                "case_loss_scaling", "case_determinism", "case_clip_errors", "case_lr_schedule"]
KERNEL_GPU_ONLY = ["big_grad_norm_full_size"]


# ---- module cases ------------------------------------------------------------------------------------------------------------
STEPS = 6
GRAD_SCALE = 0.25


def _params(dev, seed=11):
    rs = np.random.RandomState(seed)
    p0 = rs.randn(N).astype(f32)
    return p0, [torch.nn.Parameter(torch.from_numpy(c.copy()).to(dev)) for c in SC._split(p0)]


def _groups(ps, lrs=SC.LRS, wds=SC.WDS):
    return [{"params": [p], "lr": lr, "weight_decay": wd} for p, lr, wd in zip(ps, lrs, wds)]


def _make(kind, ps, capturable=False, **kw):
    if kind == "sgd":
        return step_amd.FlatSGD(_groups(ps, **kw), lr=1e-3, momentum=0.9, capturable=capturable)
    return step_amd.FlatAdam(_groups(ps, **kw), lr=1e-3, capturable=capturable)


def _arena_of(opt, t):
    """the tensors' elements of a flat arena (the arena pads every tensor to 64 elements), concatenated"""
    return np.concatenate([SC.np_(t[o:o + n]) for _, _, o, n in opt._entries])


def _load_grad(opt, g):
    """g (N elements, the tensors back to back) into the padded gradient arena"""
    off = 0
    for _, _, o, n in opt._entries:
        opt.flat_grad[o:o + n].copy_(torch.from_numpy(g[off:off + n]))
        off += n


def _gradients(seed=12, steps=STEPS):
    rs = np.random.RandomState(seed)
    return [SC._grad(rs) for _ in range(steps)]


def _against_torch(dev, kind):
    """opt.step(max_grad_norm=m, grad_scale=0.25) against torch.optim on 0.25 g preceded by torch.nn.utils.clip_grad_norm_(params, m), six
    steps on the six-segment arena; m = the median of the six gradient norms (float64 numpy, from the inputs), so three steps clip and
    three do not.  Bounds: the project's own for the same optimizers WITHOUT the clip -- parameters 2e-6 x max|p| per step
    (sgd_cases.P_BOUND), SGD's buffer sgd_cases.state_bound, Adam's moments kernel_cases.case_adam_flat's expressions.  The clip adds one
    source of difference, torch's fp32 norm against the fp64 one here (2.1e-7 relative measured between the restatement and torch, see
    case_norm_small), which scales every clipped gradient by at most that much: far inside the 1e-5 |ref| term of the state bounds.
    The returned norm, `grad_norm` and `seg_grad_norm` are checked against the restatement on the way."""
    p0, mine = _params(dev)
    ref = [torch.nn.Parameter(torch.from_numpy(c.copy())) for c in SC._split(p0)]
    grads = _gradients()
    norms = [float(np.sqrt(np.sum((g.astype(f64) * GRAD_SCALE) ** 2))) for g in grads]
    m = float(np.median(norms))
    assert sum(nv > m for nv in norms) == 3
    o = _make(kind, mine)
    o_ref = torch.optim.SGD(_groups(ref), lr=1e-3, momentum=0.9) if kind == "sgd" else torch.optim.Adam(_groups(ref), lr=1e-3)
    assert o.grad_norm is None
    clipped = 0
    for k, g in enumerate(grads):
        gs = g * f32(GRAD_SCALE)
        SC._set_grads(ref, gs)
        torch.nn.utils.clip_grad_norm_(ref, m)
        o_ref.step()
        _load_grad(o, g)
        o.step(grad_scale=GRAD_SCALE, max_grad_norm=m)
        st = SC.np_(o.grad_norm)
        tot, seg = ref_norms(g, SIZES, GRAD_SCALE)
        assert ulps(st[0], tot)[0] <= 1 and np.all(ulps(SC.np_(o.seg_grad_norm), seg) <= 1) and st[2] == 0.0, (k, st, tot)
        assert (st[1] < 1.0) == (norms[k] > m), (k, st, norms[k], m)
        clipped += int(st[1] < 1.0)
        want = np.concatenate([t.detach().numpy() for t in ref])
        got = _arena_of(o, o.flat_param)
        ep = float(np.abs(got - want).max() / np.abs(want).max())
        gc = np.concatenate([t.grad.numpy() for t in ref])                       # the clipped, scaled gradient the update saw
        if kind == "sgd":
            refb = np.concatenate([o_ref.state[t]["momentum_buffer"].numpy() for t in ref])
            err = np.abs(_arena_of(o, o.momentum_buffer) - refb)
            es = float((err / SC.state_bound(refb, gc)).max())
            ok = bool(np.all(err <= SC.state_bound(refb, gc)))
        else:
            refm = np.concatenate([o_ref.state[t]["exp_avg"].numpy() for t in ref])
            refv = np.concatenate([o_ref.state[t]["exp_avg_sq"].numpy() for t in ref])
            ga = np.abs(gc) + 1e-2
            em, ev = np.abs(_arena_of(o, o.exp_avg) - refm), np.abs(_arena_of(o, o.exp_avg_sq) - refv)
            bm, bv = 1e-5 * np.abs(refm) + 1e-6 * ga, 1e-5 * np.abs(refv) + 1e-6 * ga * ga
            es = float(max((em / bm).max(), (ev / bv).max()))
            ok = bool(np.all(em <= bm) and np.all(ev <= bv))
        print("clip + %s %s step %d: coef %.6f, max|dp|/max|p| %.3e (bound %.1e), state error / bound %.3f" % (kind, dev, k + 1, st[1], ep, SC.P_BOUND, es))
        assert ep <= SC.P_BOUND, (kind, k, ep)
        assert ok, (kind, k, es)
    assert clipped == 3
    # the method on its own: the device scalar it returns, no other norm type
    _load_grad(o, grads[0])
    r = o.clip_grad_norm_(m, grad_scale=GRAD_SCALE)
    assert isinstance(r, torch.Tensor) and r.dim() == 0 and r.device == o.flat_grad.device
    assert ulps(float(r), ref_norms(grads[0], SIZES, GRAD_SCALE)[0])[0] <= 1
    for bad in (lambda: o.clip_grad_norm_(m, norm_type=1.0), lambda: o.step(max_grad_norm=m, norm_type=float("inf"))):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("another norm type was accepted")


def case_clip_sgd_matches_torch(dev, golden):
    _against_torch(dev, "sgd")


def case_clip_adam_matches_torch(dev, golden):
    _against_torch(dev, "adam")


case_clip_sgd_matches_torch.__doc__ = case_clip_adam_matches_torch.__doc__ = _against_torch.__doc__


def case_huge_max_norm_is_no_clip(dev, golden):
    """max_grad_norm = 1e30 reproduces the trajectory without clipping BIT FOR BIT (the coefficient is exactly 1.0 and the clip pass leaves
    the arena alone), FlatSGD with momentum and FlatAdam, six steps, the fused gradient clear on some of them."""
    for kind in ("sgd", "adam"):
        arenas = []
        for m in (None, 1e30):
            _, ps = _params(dev)
            o = _make(kind, ps)
            for k, g in enumerate(_gradients()):
                _load_grad(o, g)
                o.step(grad_scale=GRAD_SCALE, zero_grad=(k % 2 == 0), max_grad_norm=m)
            assert (o.grad_norm is None) == (m is None)
            if m is not None:
                assert SC.np_(o.grad_norm)[1] == 1.0
            names = ("flat_param", "flat_grad") + (("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq"))
            arenas.append([SC.np_(getattr(o, a)) for a in names])
        assert all(np.array_equal(a, b) for a, b in zip(*arenas)), kind


def case_device_schedulers(dev, golden):
    """DeviceWarmupCosineLR / DeviceWarmupStepLR attached to a FlatSGD (momentum 0.9, capturable) over the three recorded base lrs, 40
    iterations of scheduler.step(); optimizer.step() against the same loop writing the RECORDED lr through param_groups (which reaches the
    kernel as f32(recorded lr)).  The device lr may sit 1 fp32 ulp from f32(recorded): a group's parameters are bit-equal for as long as all
    its lrs were, at least 90 % of the (iteration, group) lrs are bit-equal, and whatever diverged stays within 40 x 2^-22 x max|p| (at
    most one more rounding of p per step).  get_last_lr() returns the table and refreshes param_groups; state_dict / load_state_dict carry
    last_epoch; a second scheduler on the optimizer and a non-capturable optimizer are refused.  And a LossScaler step skipped for
    overflow still advances the schedule, not step_count."""
    gold = lr_golden()
    sizes3, iters = [64, 100, 1000], 40
    rs = np.random.RandomState(31)
    p0 = rs.randn(sum(sizes3)).astype(f32)
    grads = [SC._grad(rs, sum(sizes3)) for _ in range(iters)]
    for case in gold["cases"][:3]:
        a = dict(case["args"])
        cls = step_amd.DeviceWarmupCosineLR if case["kind"] == "cosine" else step_amd.DeviceWarmupStepLR
        pair = []
        for _ in range(2):
            ps = [torch.nn.Parameter(torch.from_numpy(c.copy()).to(dev)) for c in SC._split(p0, sizes3)]
            pair.append((ps, step_amd.FlatSGD([{"params": [p], "lr": lr} for p, lr in zip(ps, gold["base_lrs"])], lr=1e-3, momentum=0.9,
                                              weight_decay=1e-4, capturable=True)))
        (ps_d, o_d), (ps_h, o_h) = pair
        sch = cls(o_d, **a)
        assert sch.last_epoch == 0 and o_d.lr_scheduler is sch and sch.base_lrs == gold["base_lrs"]
        alive, pairs_equal = [True, True, True], 0
        for k in range(1, iters + 1):
            for g_, lr in zip(o_h.param_groups, case["lrs"][k]):
                g_["lr"] = lr
            for o in (o_d, o_h):
                for p, c in zip(o.param_groups, SC._split(grads[k - 1], sizes3)):
                    p["params"][0].grad.copy_(torch.from_numpy(c))
            sch.step()
            o_d.step(zero_grad=True)
            o_h.step(zero_grad=True)
            d = ulps(SC.np_(o_d._seg_lr), np.array(case["lrs"][k]).astype(f32))
            assert d.max() <= 1 and np.array_equal(SC.np_(o_h._seg_lr), np.array(case["lrs"][k]).astype(f32)), (case["name"], k)
            for i in range(3):
                alive[i] = alive[i] and d[i] == 0
                pairs_equal += int(d[i] == 0)
                if alive[i]:
                    assert torch.equal(ps_d[i].detach(), ps_h[i].detach()), (case["name"], k, i)
        print("device scheduler %s %s: %d of %d (iteration, group) lrs bit-equal" % (case["name"], dev, pairs_equal, 3 * iters))
        assert pairs_equal >= 0.9 * 3 * iters, (case["name"], pairs_equal)
        pm = max(float(p.detach().abs().max()) for p in ps_h)
        for p, q in zip(ps_d, ps_h):
            assert float((p.detach() - q.detach()).abs().max()) <= iters * 2.0 ** -22 * pm
        assert sch.last_epoch == iters and o_d.step_count == iters
        last = sch.get_last_lr()
        assert last == SC.np_(o_d._seg_lr).tolist() and [g_["lr"] for g_ in o_d.param_groups] == last
        assert sch.state_dict() == {"last_epoch": iters}
        sch.load_state_dict({"last_epoch": 7})
        assert sch.last_epoch == 7 and np.all(ulps(SC.np_(o_d._seg_lr), np.array(case["lrs"][7]).astype(f32)) <= 1)
        try:
            cls(o_d, **a)
        except RuntimeError:
            pass
        else:
            raise AssertionError("a second device scheduler was accepted")
    # resumed: constructed at last_epoch 45 it continues the recorded sequence
    case = gold["cases"][3]
    ps = [torch.nn.Parameter(torch.zeros(s).to(dev)) for s in sizes3]
    o = step_amd.FlatSGD([{"params": [p], "lr": lr, "initial_lr": lr} for p, lr in zip(ps, gold["base_lrs"])], lr=1e-3, momentum=0.9, capturable=True)
    sch = step_amd.DeviceWarmupCosineLR(o, last_epoch=case["last_epoch"], **case["args"])
    for k in range(5):
        assert sch.last_epoch == case["first_epoch"] + k
        assert np.all(ulps(SC.np_(o._seg_lr), np.array(case["lrs"][k]).astype(f32)) <= 1), k
        sch.step()
    try:
        step_amd.DeviceWarmupStepLR(step_amd.FlatSGD([torch.nn.Parameter(torch.zeros(8).to(dev))], lr=0.1), [5])
    except RuntimeError:
        pass
    else:
        raise AssertionError("a device scheduler on a non-capturable optimizer was accepted")
    # a step the loss scaler skips still advances the schedule, not the optimizer's count
    scaler = step_amd.LossScaler(dev, init_scale=1024.0)
    before = (sch.last_epoch, o.step_count, SC.np_(o.flat_param).copy())
    o.flat_grad.fill_(1.0)
    o.flat_grad[3] = float("inf")
    sch.step()
    o.step(scaler=scaler, zero_grad=True, max_grad_norm=1.0)
    assert SC.np_(o.grad_norm)[2] == 1.0 and SC.np_(o.grad_norm)[1] == 1.0
    assert sch.last_epoch == before[0] + 1 and o.step_count == before[1] and np.array_equal(SC.np_(o.flat_param), before[2])
    assert scaler.scale == 512.0
    o.flat_grad.fill_(1024.0 * 0.5)
    sch.step()
    o.step(scaler=scaler, zero_grad=True, max_grad_norm=1.0)                    # clean: clipped in un-scaled units (|g| = 1 per element)
    n_el = float(o.numel)
    assert ulps(SC.np_(o.grad_norm)[0], f32(np.sqrt(n_el)))[0] <= 1 and o.step_count == before[1] + 1 and sch.last_epoch == before[0] + 2


MODULE_CASES = ["case_clip_sgd_matches_torch", "case_clip_adam_matches_torch", "case_huge_max_norm_is_no_clip", "case_device_schedulers"]
