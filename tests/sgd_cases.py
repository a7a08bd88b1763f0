"""Cases for the SGD-with-momentum path (step_sgd_flat / _dev / _amp, step_amd.FlatSGD), driven on the host interpreter by
tests/test_emul_sgd.py and on the real library by tests/test_gpu_sgd.py.  The reference of every comparison is torch.optim.SGD
itself -- what train.py:124 constructs -- run inside the case.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import ctypes
import hashlib

import numpy as np
import torch

import step_amd

f32 = np.float32

# the arena of kernel_cases.case_adam_flat: six segments with their own lr / weight decay
SIZES = [12, 64, 4, 100, 28, 1000]
LRS = [1e-3, 2e-3, 5e-4, 1e-3, 1e-2, 3e-4]
WDS = [0.0, 1e-2, 0.0, 1e-4, 0.0, 1e-7]
N = sum(SIZES)
GRAD_SCALE = 0.25
STEPS = 6

# (momentum, dampening, nesterov) and the factor on the project's state bound (see case_sgd_flat's docstring)
VARIANTS = {"momentum": (0.9, 0.0, 0, 1.0), "nesterov": (0.9, 0.0, 1, 1.0), "dampening": (0.9, 0.1, 0, 2.2), "plain": (0.0, 0.0, 0, 1.0)}
P_BOUND = 2e-6                                               # x max|p|, per step


def state_bound(ref, g_scaled, k=1.0):
    """the project's bound for an optimizer state against torch (kernel_cases.case_adam_flat): a few ulp of the operands"""
    return k * (1e-5 * np.abs(ref) + 1e-6 * (np.abs(g_scaled) + 1e-2))


def _split(a, sizes=SIZES):
    out, off = [], 0
    for s in sizes:
        out.append(a[off:off + s])
        off += s
    return out


def _torch_sgd(p0, sizes, lrs, wds, momentum, dampening, nesterov):
    tp = [torch.nn.Parameter(torch.from_numpy(c.copy())) for c in _split(p0, sizes)]
    opt = torch.optim.SGD([{"params": [t], "lr": lr, "weight_decay": wd} for t, lr, wd in zip(tp, lrs, wds)], lr=1e-3, momentum=momentum,
                          dampening=dampening, nesterov=bool(nesterov))
    return tp, opt


def _set_grads(tp, g, sizes=SIZES):
    for t, c in zip(tp, _split(g, sizes)):
        t.grad = torch.from_numpy(c.copy())


def _ref_arenas(tp, opt, momentum):
    ref = np.concatenate([t.detach().numpy() for t in tp])
    refb = np.concatenate([opt.state[t]["momentum_buffer"].numpy() for t in tp]) if momentum != 0 else None
    return ref, refb


def _grad(rs, n=N):
    return (rs.randn(n) * (10.0 ** rs.uniform(-4, 1, n))).astype(f32)        # magnitudes 1e-4 .. 1e1


def _addr(ptr):
    return ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr)


def _shift(ptr, nbytes):
    return ctypes.c_void_p(_addr(ptr) + nbytes)


def _sgd_flat(bk, variant):
    """step_sgd_flat against torch.optim.SGD over single-tensor groups with their own lr / weight decay (utils/solver.py:12-93), six
    steps (the buffer recurrence runs five times past its initialisation), grad_scale 0.25, the fused clear on four of the six steps;
    step_sgd_flat_dev on a twin set of arenas BIT FOR BIT equal at every step, its counter reading 1, 2, 3, ...

    Bounds.  SGD is adds and multiplies only; the one legitimate difference from torch is whether a multiply-add pair is contracted into
    an FMA (torch's CPU `add_(alpha=)` is: buf*mu is rounded, then fma(alpha, g, .)).  Observed for an UNFUSED numpy restatement of
    the five lines of _single_tensor_sgd against torch.optim.SGD on the CPU, these inputs, all elements, maximum over the six steps:
        variant      max|dp| / max|p|   (bound 2e-6)     max state error / (1e-5 |ref| + 1e-6 (|g s| + 1e-2))
        momentum     3.4e-08                              0.028
        nesterov     3.4e-08                              0.020
        dampening    4.3e-09                              0.533
        plain        0 (bit-identical)                    -
    Parameters: the project's 2e-6 x max|p| is > 50x the observation, kept.  State: kept where the observation is >= 4x inside
    (momentum, nesterov); with dampening 0.1 it is not -- (1 - dampening) * g is a second rounded product per step whose error the
    recurrence carries along while buf itself may cancel to well below the gradients that fed it -- so that variant's bound is 4 x 0.533
    = 2.2 x the project's expression.  None of these figures comes from the kernels under test."""
    momentum, dampening, nesterov, kb = VARIANTS[variant]
    rs = np.random.RandomState(11)
    p0 = rs.randn(N).astype(f32)
    tp, opt = _torch_sgd(p0, SIZES, LRS, WDS, momentum, dampening, nesterov)
    mom = momentum != 0
    P, P2 = bk.dev(p0.copy()), bk.dev(p0.copy())
    B, B2 = bk.dev(np.zeros(N, f32) if mom else None), bk.dev(np.zeros(N, f32) if mom else None)     # momentum 0: NULL buffer
    ends = bk.dev(np.cumsum(SIZES).astype(np.int64))
    LR, WD = bk.dev(np.array(LRS, f32)), bk.dev(np.array(WDS, f32))
    cnt = bk.dev(np.zeros(1, np.int64))
    for step_no in range(1, STEPS + 1):
        g = _grad(rs)
        _set_grads(tp, g * f32(GRAD_SCALE))
        opt.step()
        G, G2 = bk.dev(g.copy()), bk.dev(g.copy())
        zero = int(step_no not in (2, 5))
        assert bk.lib.step_sgd_flat(P.ptr, G.ptr, B.ptr, N, ends.ptr, LR.ptr, WD.ptr, len(SIZES), momentum, dampening, nesterov, step_no,
                                    GRAD_SCALE, zero, bk.stream) == 0
        ref, refb = _ref_arenas(tp, opt, momentum)
        ep = float(np.abs(P.get() - ref).max() / np.abs(ref).max())
        es = float((np.abs(B.get() - refb) / state_bound(refb, g * f32(GRAD_SCALE))).max()) if mom else 0.0
        print("sgd_flat[%s] %s step %d: max|dp|/max|p| %.3e (bound %.1e), state error / bound %.3f (allowed %.1f)"
              % (variant, bk.name, step_no, ep, P_BOUND, es, kb))
        assert ep <= P_BOUND, (variant, step_no, ep)
        if mom:
            assert np.all(np.abs(B.get() - refb) <= state_bound(refb, g * f32(GRAD_SCALE), kb)), (variant, step_no, es)
        assert np.array_equal(G.get(), np.zeros(N, f32) if zero else g), (variant, step_no)          # exactly zero / exactly untouched
        assert bk.lib.step_sgd_flat_dev(P2.ptr, G2.ptr, B2.ptr, N, ends.ptr, LR.ptr, WD.ptr, len(SIZES), momentum, dampening, nesterov,
                                        cnt.ptr, GRAD_SCALE, zero, bk.stream) == 0
        assert int(cnt.get()[0]) == step_no
        assert np.array_equal(P2.get(), P.get()) and np.array_equal(G2.get(), G.get()), (variant, step_no)
        if mom:
            assert np.array_equal(B2.get(), B.get()), (variant, step_no)


def case_sgd_flat_momentum(bk, golden):
    _sgd_flat(bk, "momentum")


def case_sgd_flat_nesterov(bk, golden):
    _sgd_flat(bk, "nesterov")


def case_sgd_flat_dampening(bk, golden):
    _sgd_flat(bk, "dampening")


def case_sgd_flat_plain(bk, golden):
    _sgd_flat(bk, "plain")


for _f in (case_sgd_flat_momentum, case_sgd_flat_nesterov, case_sgd_flat_dampening, case_sgd_flat_plain):
    _f.__doc__ = _sgd_flat.__doc__


def case_sgd_flat_amp(bk, golden):
    """step_sgd_flat_amp -- dynamic loss scaling on the device -- with an OVERFLOW ON THE VERY FIRST STEP: the skipped step leaves
    parameters, buffer and counter as they are (gradients cleared when asked, scale halved, tracker reset), and the first CLEAN step
    that follows initialises the buffer with buf = g, not with the recurrence.  Dampening 0.1 and a buffer arena that starts out holding
    777 make the two distinguishable (momentum * 0 + 1 * g would hide the difference).  Clean steps equal step_sgd_flat_dev with
    grad_scale / scale bit for bit (the twin is simply not called on an overflow iteration), and both follow a torch.optim.SGD that was
    not stepped on the overflow iterations (torch.amp.GradScaler.step skips optimizer.step()), within the bounds of case_sgd_flat's
    dampening variant.  A nan later on skips as well; the scale grows after `interval` clean steps in a row."""
    rs = np.random.RandomState(5)
    sizes, lrs, wds = [64, 8, 256], [1e-3, 2e-3, 5e-4], [0.0, 1e-2, 0.0]
    n = sum(sizes)
    momentum, dampening, nesterov, kb = VARIANTS["dampening"]
    p0 = rs.randn(n).astype(f32)
    tp, opt = _torch_sgd(p0, sizes, lrs, wds, momentum, dampening, nesterov)
    ends = bk.dev(np.cumsum(sizes).astype(np.int64))
    LR, WD = bk.dev(np.array(lrs, f32)), bk.dev(np.array(wds, f32))
    P, B = bk.dev(p0.copy()), bk.dev(np.full(n, 777.0, f32))
    P2, B2 = bk.dev(p0.copy()), bk.dev(np.full(n, 777.0, f32))
    cnt, cnt2 = bk.dev(np.zeros(1, np.int64)), bk.dev(np.zeros(1, np.int64))
    amp = bk.dev(np.array([1024.0, 0.0, 0.0, 0.0], f32))
    scale, tracker, steps = 1024.0, 0, 0
    interval = 3
    plan = ["inf", "ok", "ok", "nan", "ok", "ok", "ok", "ok"]          # overflow first; growth after 3 clean steps in a row
    for k, kind in enumerate(plan):
        g = (rs.randn(n) * 0.1).astype(f32)
        gs = (g * f32(scale)).astype(f32)                             # what backward of the scaled loss leaves in the arena
        if kind == "inf":
            gs[17] = np.inf
        elif kind == "nan":
            gs[n - 3] = np.nan
        G = bk.dev(gs.copy())
        before = (P.get().copy(), B.get().copy())
        zero = int(k % 2 == 0)
        assert bk.lib.step_sgd_flat_amp(P.ptr, G.ptr, B.ptr, n, ends.ptr, LR.ptr, WD.ptr, len(sizes), momentum, dampening, nesterov, cnt.ptr,
                                        0.5, zero, amp.ptr, 2.0, 0.5, interval, bk.stream) == 0
        if kind == "ok":
            G2 = bk.dev(gs.copy())
            gscale = 0.5 * (1.0 / scale)
            assert bk.lib.step_sgd_flat_dev(P2.ptr, G2.ptr, B2.ptr, n, ends.ptr, LR.ptr, WD.ptr, len(sizes), momentum, dampening, nesterov,
                                            cnt2.ptr, gscale, zero, bk.stream) == 0
            assert np.array_equal(P.get(), P2.get()) and np.array_equal(B.get(), B2.get()), k
            gu = gs * f32(gscale)                                     # (scale is a power of two: exactly g / 2)
            _set_grads(tp, gu, sizes)
            opt.step()
            ref, refb = _ref_arenas(tp, opt, momentum)
            assert np.abs(P.get() - ref).max() <= P_BOUND * np.abs(ref).max(), k
            assert np.all(np.abs(B.get() - refb) <= state_bound(refb, gu, kb)), (k, float(np.abs(B.get() - refb).max()))
            steps += 1
            tracker += 1
            if tracker == interval:
                scale, tracker = scale * 2.0, 0
        else:
            assert all(np.array_equal(a, b) for a, b in zip(before, (P.get(), B.get()))), k              # skipped: nothing moved
            scale, tracker = scale * 0.5, 0
        assert int(cnt.get()[0]) == steps, (k, cnt.get(), steps)
        st = amp.get()
        assert st[0] == f32(scale) and st[1] == f32(tracker) and st[2] == 0.0, (k, st, scale, tracker)
        if zero:
            assert not G.get().any(), k
        else:
            assert np.array_equal(G.get(), gs, equal_nan=True), k
    assert steps == 6 and scale == 1024.0 * 0.5 * 0.5 * 2.0


def case_sgd_flat_errors(bk, golden):
    """Argument errors of the three entry points: negative status and NOTHING written (arenas, counter and loss-scale state are
    compared with their copies afterwards); n == 0 succeeds (and, on the device-counted form, still counts as a step, as Adam's)."""
    rs = np.random.RandomState(3)
    n = N
    p0, g0, b0 = rs.randn(n).astype(f32), rs.randn(n).astype(f32), rs.randn(n).astype(f32)
    P, G, B = bk.dev(p0.copy()), bk.dev(g0.copy()), bk.dev(b0.copy())
    ends = bk.dev(np.cumsum(SIZES).astype(np.int64))
    LR, WD = bk.dev(np.array(LRS, f32)), bk.dev(np.array(WDS, f32))
    cnt = bk.dev(np.full(1, 4, np.int64))
    amp = bk.dev(np.array([512.0, 1.0, 0.0, 0.0], f32))
    ns, L, s = len(SIZES), bk.lib, bk.stream

    def flat(p=P.ptr, g=G.ptr, b=B.ptr, n_=n, nseg=ns, mu=0.9, damp=0.0, nest=0, step=2):
        return L.step_sgd_flat(p, g, b, n_, ends.ptr, LR.ptr, WD.ptr, nseg, mu, damp, nest, step, 1.0, 1, s)

    def dev(p=P.ptr, g=G.ptr, b=B.ptr, n_=n, nseg=ns, mu=0.9, damp=0.0, nest=0, c=cnt.ptr):
        return L.step_sgd_flat_dev(p, g, b, n_, ends.ptr, LR.ptr, WD.ptr, nseg, mu, damp, nest, c, 1.0, 1, s)

    def amp_(p=P.ptr, g=G.ptr, b=B.ptr, n_=n, nseg=ns, mu=0.9, damp=0.0, nest=0, c=cnt.ptr, a=amp.ptr, growth=2.0, backoff=0.5, interval=3):
        return L.step_sgd_flat_amp(p, g, b, n_, ends.ptr, LR.ptr, WD.ptr, nseg, mu, damp, nest, c, 1.0, 1, a, growth, backoff, interval, s)

    for fn in (flat, dev, amp_):
        assert fn(n_=n + 2) < 0                                                    # n % 4
        assert fn(n_=-4) < 0
        assert fn(p=None) < 0 and fn(g=None) < 0 and fn(b=None) < 0                # NULL arenas (momentum != 0 needs its buffer)
        assert fn(p=_shift(P.ptr, 4)) < 0 and fn(g=_shift(G.ptr, 8)) < 0 and fn(b=_shift(B.ptr, 4)) < 0      # 16-byte alignment
        assert fn(nseg=0) < 0 and fn(nseg=4097) < 0                                # n_seg out of range
        assert fn(mu=0.0, nest=1) < 0                                              # nesterov without momentum
        assert fn(mu=0.9, damp=0.1, nest=1) < 0                                    # nesterov with dampening
        assert fn(mu=-0.5) < 0
    assert flat(step=0) < 0                                                        # steps count from 1
    assert dev(c=None) < 0 and amp_(c=None) < 0                                    # NULL step_dev
    assert amp_(a=None) < 0
    assert amp_(interval=0) < 0 and amp_(growth=0.5) < 0 and amp_(backoff=1.5) < 0
    assert np.array_equal(P.get(), p0) and np.array_equal(G.get(), g0) and np.array_equal(B.get(), b0)
    assert int(cnt.get()[0]) == 4 and np.array_equal(amp.get(), np.array([512.0, 1.0, 0.0, 0.0], f32))
    # n == 0: success, no arena is touched (NULL arenas are fine then)
    assert flat(p=None, g=None, b=None, n_=0) == 0
    assert dev(p=None, g=None, b=None, n_=0) == 0 and int(cnt.get()[0]) == 5
    assert np.array_equal(P.get(), p0) and np.array_equal(G.get(), g0) and np.array_equal(B.get(), b0)
    # momentum == 0: the buffer may be NULL and, when given, is neither read nor written
    assert flat(b=None, mu=0.0) == 0
    assert np.array_equal(B.get(), b0) and not G.get().any() and not np.array_equal(P.get(), p0)


def big_sgd_full_size(bk, golden):
    """The fused SGD at the C4 parameter count (the sizes of kernel_cases.big_adam_full_size, 44.4 M fp32) against torch.optim.SGD on the
    same device: 2 steps, momentum 0.9, per-segment lr / weight decay, gradient arena cleared.  Bounds of case_sgd_flat (torch's device
    kernels may contract a multiply-add where this kernel does not, or the other way round: one rounding per operation), all elements."""
    torch.manual_seed(3)
    sizes = [4_000_000 + 64 * i for i in range(11)]
    n = sum(sizes)
    assert abs(n - 44_422_936) < 500_000
    ps = [torch.nn.Parameter(torch.randn(s_, device="cuda") * 0.05) for s_ in sizes]
    lrs = [1e-3 * (1 + i % 3) for i in range(len(sizes))]
    wds = [0.0 if i % 2 else 1e-4 for i in range(len(sizes))]
    opt = torch.optim.SGD([{"params": [p], "lr": lr, "weight_decay": wd} for p, lr, wd in zip(ps, lrs, wds)], lr=1e-3, momentum=0.9)
    P = torch.cat([p.detach().reshape(-1) for p in ps]).clone()
    B = torch.zeros_like(P)
    ends = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device="cuda")
    LR, WD = torch.tensor(lrs, device="cuda"), torch.tensor(wds, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for step_no in (1, 2):
        G = torch.randn(n, device="cuda")
        ga = G.abs()
        off = 0
        for p, s_ in zip(ps, sizes):
            p.grad = G[off:off + s_].clone()
            off += s_
        opt.step()
        assert bk.lib.step_sgd_flat(vp(P), vp(G), vp(B), n, vp(ends), vp(LR), vp(WD), len(sizes), 0.9, 0.0, 0, step_no, 1.0, 1, bk.stream) == 0
        ref = torch.cat([p.detach().reshape(-1) for p in ps])
        refb = torch.cat([opt.state[p]["momentum_buffer"].reshape(-1) for p in ps])
        ep = float((P - ref).abs().max()) / float(ref.abs().max())
        es = float(((B - refb).abs() / (1e-5 * refb.abs() + 1e-6 * (ga + 1e-2))).max())
        print("big_sgd_full_size step %d: max|dp|/max|p| %.3e (bound %.1e), state error / bound %.3f (allowed 1)" % (step_no, ep, P_BOUND, es))
        assert ep <= P_BOUND, (step_no, ep)
        assert es <= 1.0, (step_no, es)
        assert float(G.abs().max()) == 0.0


KERNEL_CASES = ["case_sgd_flat_momentum", "case_sgd_flat_nesterov", "case_sgd_flat_dampening", "case_sgd_flat_plain", "case_sgd_flat_amp",
                "case_sgd_flat_errors"]
KERNEL_GPU_ONLY = ["big_sgd_full_size"]


# ---- module cases ------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def np_(t):
    return t.detach().float().cpu().contiguous().numpy()


def case_flat_sgd_matches_torch(dev, golden):
    """step_amd.FlatSGD against torch.optim.SGD (train.py:124) on the parameter groups utils/solver.py builds (bias: 2x lr, no decay):
    three steps with an lr change in between through a torch LambdaLR (the reference's schedulers are _LRScheduler subclasses), a
    replaced .grad, grad_scale, the fused gradient clear, the autograd version bump; then the state_dict of each side loaded into a
    fresh optimizer of the OTHER class, after which both pairs take one more step and still agree; constructor refusals.
    Tolerances: parameters 2e-6 x max|p| per step and buffers 1e-5 x max|buf| -- the project's figures for the same comparison of FlatAdam
    (module_cases.case_flat_adam_matches_torch), which SGD's shorter arithmetic meets with room (see case_sgd_flat)."""
    torch.manual_seed(5)
    shapes = [(7, 3, 1, 3, 3), (7,), (5, 7), (5,), (130,)]
    ref = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref]
    kw = dict(lr=1e-3, momentum=0.9, weight_decay=1e-7)

    def groups(ps):
        return [{"params": [p], "lr": 2e-3 if p.dim() == 1 else 1e-3, "weight_decay": 0 if p.dim() == 1 else 1e-4} for p in ps]

    o_ref = torch.optim.SGD(groups(ref), **kw)
    o = step_amd.FlatSGD(groups(mine), **kw)
    assert isinstance(o, torch.optim.Optimizer)
    assert len(o.param_groups) == len(o_ref.param_groups) and o.param_groups[1]["lr"] == 2e-3
    assert {k: v for k, v in o.param_groups[0].items() if k != "params"} == {k: v for k, v in o_ref.param_groups[0].items() if k != "params"}
    assert o.state_dict()["state"] == {} and o.step_count == 0
    sch = [torch.optim.lr_scheduler.LambdaLR(x, lambda k: 0.5 if k == 1 else 1.0) for x in (o_ref, o)]
    for p, q in zip(ref, mine):
        assert torch.equal(p.detach(), q.detach().cpu())         # re-homing into the arena keeps the values

    def backward_both(it, replace=None):
        for i, (p, q) in enumerate(zip(ref, mine)):
            w = torch.randn(p.shape)
            (p * w).sum().mul(3.0).backward()
            if replace == i:
                q.grad = (w * 1.5).to(dev)                       # a caller that replaced .grad (not halved below, hence 1.5)
            else:
                (q * w.to(dev)).sum().mul(3.0).backward()

    def buffers(opt_, ps):
        return np.concatenate([np_(opt_.state[p]["momentum_buffer"]).reshape(-1) for p in ps])

    def mine_buffers(opt_):
        return np.concatenate([np_(opt_.momentum_buffer[o_:o_ + n_]) for _, _, o_, n_ in opt_._entries])

    for it in range(3):
        assert [g_["lr"] for g_ in o.param_groups] == [g_["lr"] for g_ in o_ref.param_groups]
        assert o.param_groups[0]["lr"] == (5e-4 if it == 1 else 1e-3)
        o_ref.zero_grad()
        if it != 2:
            o.zero_grad()                                        # it == 2 relies on the clear fused into step 1
        vers = [q._version for q in mine]
        backward_both(it, replace=2 if it == 0 else None)
        o_ref.step()
        if it == 0:
            assert mine[2].grad.data_ptr() != o.flat_grad.data_ptr() + 4 * 256       # step() folds it back into the arena
        o.flat_grad.mul_(0.5)                                    # grad_scale 2 on halved gradients == the same update
        o.step(grad_scale=2.0, zero_grad=(it == 1))
        for x in sch:
            x.step()
        assert mine[2].grad.data_ptr() == o.flat_grad.data_ptr() + 4 * 256       # 189 -> 192, 7 -> 64 elements before it
        assert o.step_count == it + 1
        for p, q, v in zip(ref, mine, vers):
            assert q._version > v
            assert rel(np_(q), p.detach().numpy()) < 2e-6, (it, tuple(p.shape))
        assert rel(mine_buffers(o), buffers(o_ref, ref)) < 1e-5, it
        if it == 1:
            assert float(o.flat_grad.abs().max()) == 0.0
    # FlatSGD's state_dict INTO torch's SGD, torch's INTO a fresh FlatSGD; both then take one more step
    sd = o.state_dict()
    assert sorted(sd["state"]) == list(range(len(shapes))) and set(sd["state"][0]) == {"momentum_buffer"}
    assert set(sd["param_groups"][0]) == set(o_ref.state_dict()["param_groups"][0])
    t_par = [torch.nn.Parameter(q.detach().cpu().clone()) for q in mine]
    o2 = torch.optim.SGD(groups(t_par), **kw)
    o2.load_state_dict({"state": {k: {kk: vv.cpu() for kk, vv in st.items()} for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]})
    assert rel(buffers(o2, t_par), buffers(o_ref, ref)) < 1e-5
    f_par = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref]
    o3 = step_amd.FlatSGD(groups(f_par), **kw)
    o3.load_state_dict(o_ref.state_dict())
    assert o3.step_count >= 1 and rel(mine_buffers(o3), buffers(o_ref, ref)) < 1e-5
    assert o3.param_groups[0]["lr"] == o_ref.param_groups[0]["lr"]
    o_ref.zero_grad()
    for x in (o, o2, o3):
        x.zero_grad()
    for p, q, t_, f_ in zip(ref, mine, t_par, f_par):
        w = torch.randn(p.shape)
        (p * w).sum().mul(3.0).backward()
        (q * w.to(dev)).sum().mul(3.0).backward()
        (t_ * w).sum().mul(3.0).backward()
        (f_ * w.to(dev)).sum().mul(3.0).backward()
    for x in (o_ref, o, o2, o3):
        x.step()
    for p, q, t_, f_ in zip(ref, mine, t_par, f_par):
        want = p.detach().numpy()
        assert rel(np_(q), want) < 2e-6 and rel(np_(t_), want) < 2e-6 and rel(np_(f_), want) < 2e-6, tuple(p.shape)
    assert rel(mine_buffers(o3), buffers(o_ref, ref)) < 1e-5 and rel(buffers(o2, t_par), buffers(o_ref, ref)) < 1e-5
    # a dict without buffers resets the count: the next step initialises the buffer again
    fresh = torch.optim.SGD(groups([torch.nn.Parameter(p.detach().clone()) for p in ref]), **kw)
    o3.load_state_dict(fresh.state_dict())
    assert o3.step_count == 0 and float(o3.momentum_buffer.abs().max()) == 0.0 and o3.state_dict()["state"] == {}
    # momentum 0: no buffer arena, no state (torch keeps none either)
    o4 = step_amd.FlatSGD([torch.nn.Parameter(torch.randn(8).to(dev))], lr=0.1)
    assert o4.momentum_buffer is None
    o4.step()
    assert o4.state_dict()["state"] == {} and o4.step_count == 1
    # refusals
    for bad, exc in ((lambda: step_amd.FlatSGD([{"params": [torch.nn.Parameter(torch.randn(4).to(dev))], "momentum": 0.5},
                                                {"params": [torch.nn.Parameter(torch.randn(4).to(dev))]}], lr=0.1, momentum=0.9), ValueError),
                     (lambda: step_amd.FlatSGD([torch.nn.Parameter(torch.randn(4).to(dev).half())], lr=0.1), RuntimeError),
                     (lambda: step_amd.FlatSGD([torch.nn.Parameter(torch.randn(4).to(dev))], lr=0.1, nesterov=True), ValueError),
                     (lambda: step_amd.FlatSGD([torch.nn.Parameter(torch.randn(4).to(dev))], lr=0.1, momentum=0.9).step(scaler=object()), RuntimeError)):
        try:
            bad()
        except exc:
            continue
        raise AssertionError("FlatSGD accepted a bad argument")


# FlatAdam on the host interpreter at the commit BEFORE the optimizers were given a common base class: recorded by running
# adam_trajectory("cpu") below, under tests.emul.patch.emulated_kernels, in a checkout of that commit (3b0f25c; the interpreter build is
# -O2 -ffp-contract=off host code and the inputs come from numpy's RandomState, so the run is deterministic).
ADAM_PARENT = {
    "attributes": ["_bias_corr", "_entries", "_seg_end", "_seg_lr", "_seg_wd", "_step_dev", "_step_host", "_tables", "capturable", "device",
                   "exp_avg", "exp_avg_sq", "flat_grad", "flat_param", "numel"],
    "state_dict_keys": {"top": ["param_groups", "state"], "state": [0, 1, 2, 3, 4], "entry": ["exp_avg", "exp_avg_sq", "step"],
                        "group": ["betas", "eps", "lr", "params", "weight_decay"]},
    "hashes": ["f75b992df8d002309d69430b6a9c461f25ce98e2a30e5a7037eb4880e9bfd83c",
               "3e792e0f465ac6a0edd8d470fe422b43694baa2a798ec1daf384992f10819d55",
               "179527978e5c6f252e2898d3809ac35312b00bb4e4b9e140bf0b4578396c95c4"],
}


class _PlainOptimizer(torch.optim.Optimizer):
    """what torch.optim.Optimizer itself leaves on an instance (hook tables, defaults, param_groups, state: names that follow the torch
    version, not this project)"""


def adam_trajectory(dev):
    """Three FlatAdam steps on fixed inputs: (sorted instance attributes beyond torch.optim.Optimizer's own, state_dict keys, sha256 of
    flat_param + exp_avg + exp_avg_sq after each step)."""
    rs = np.random.RandomState(2024)
    shapes = [(7, 3, 1, 3, 3), (7,), (5, 7), (5,), (130,)]
    ps = [torch.nn.Parameter(torch.from_numpy(rs.randn(*s).astype(f32)).to(dev)) for s in shapes]
    o = step_amd.FlatAdam([{"params": [p], "lr": 2e-3 if p.dim() == 1 else 1e-3, "weight_decay": 0 if p.dim() == 1 else 1e-4} for p in ps], lr=1e-3)
    hashes = []
    for it in range(3):
        for p in ps:
            p.grad.copy_(torch.from_numpy((rs.randn(*p.shape) * 10.0 ** rs.uniform(-3, 1)).astype(f32)))
        if it == 1:
            for g_ in o.param_groups:
                g_["lr"] *= 0.5
        o.step(grad_scale=0.5, zero_grad=(it != 1))
        h = hashlib.sha256()
        for a in (o.flat_param, o.exp_avg, o.exp_avg_sq):
            h.update(np_(a).tobytes())
        hashes.append(h.hexdigest())
    sd = o.state_dict()
    keys = {"top": sorted(sd), "state": sorted(sd["state"]), "entry": sorted(sd["state"][0]), "group": sorted(sd["param_groups"][0])}
    own = set(vars(o)) - set(vars(_PlainOptimizer([torch.nn.Parameter(torch.zeros(1))], {})))
    return sorted(own), keys, hashes


def case_flat_adam_unchanged(dev, golden):
    """The common base class changed nothing about FlatAdam: the names of its instance attributes (flat_param, flat_grad, exp_avg,
    exp_avg_sq, _entries, _step_dev, capturable, ... -- step_amd.dist, step_amd.workloads and tools/ read them), the keys of its
    state_dict() and a three-step trajectory are what the parent commit produces; on the interpreter the trajectory is compared BIT FOR
    BIT through the recorded hashes (the GPU's arithmetic may contract differently from the host build, so there only names and keys)."""
    attrs, keys, hashes = adam_trajectory(dev)
    assert attrs == ADAM_PARENT["attributes"], sorted(set(attrs) ^ set(ADAM_PARENT["attributes"]))
    assert keys == ADAM_PARENT["state_dict_keys"]
    if dev == "cpu":
        assert hashes == ADAM_PARENT["hashes"], hashes
    assert len(set(hashes)) == 3


MODULE_CASES = ["case_flat_sgd_matches_torch", "case_flat_adam_unchanged"]
