"""Cases for the bf16 gradient wire with error feedback (step_grad_pack16 / step_grad_unpack16, step_amd.dist.GradWire, the wire= forms of
BucketedReducer and allreduce_flat), driven on the host interpreter by tests/test_emul_wire.py and on the real library by
tests/test_gpu_wire.py.

The reference of every kernel comparison is the numpy restatement below, written from the definition in include/step_amd.h and using
nothing of the product: v = g * s + r in float32 (ONE rounding where g * s is exact: s a power of two), round to nearest even to
bfloat16 as ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) on the bit pattern, residual v - widen(w) in float32, 0 where w is inf / NaN.
Everything is compared for EQUALITY of bit patterns: the residual of a round-to-nearest-even to bfloat16 is exactly representable in
float32 (asserted of the restatement itself: widen(w) + r == v bitwise), there is nothing to tolerate.  The one bounded comparison is
pre_scale = 3, where a float64 restatement can double-round: there the kernel's own v' = widen(w) + r' must lie within one float32 ulp
of the float64 3 g + r (a fused multiply-add is correctly rounded: half an ulp; one ulp is what the issue sets) and w must be rne(v').
Inputs keep |v| >= 2^-126 or zero: what the conversion does with float32 subnormals is not part of the contract.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda") and run
inside a ONE-rank gloo group that the case sets up itself (file:// store), with single_rank=True so that the exchange is active."""
import contextlib
import ctypes
import os
import tempfile

import numpy as np
import torch

from step_amd import _capi

F32, BF16, F16 = _capi.F32, _capi.BF16, _capi.F16
E_SHAPE, E_NULL, E_UNSUPPORTED = -2, -3, -4
u64 = np.uint64
GUARD = 16                                                       # elements in front of and behind every tensor handed to a kernel

SIZES = [0, 1, 7, 8, 9, 2368, 65536 + 3]                         # nothing; lone tail; under / at / over one vector; one block + grid-stride; several passes + tail
PLANTED = np.array([0.0, -0.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 3 * 2.0 ** -8, 3.4e38, np.inf, -np.inf, np.nan], np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def rne(v):
    """float32 -> bfloat16 bits, round to nearest even (NaN inputs give some value: callers compare those by isnan)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(u64)
    return ((u + u64(0x7FFF) + ((u >> u64(16)) & u64(1))) >> u64(16)).astype(np.uint16)


def widen(w):
    return (np.asarray(w).astype(np.uint32) << np.uint32(16)).view(np.float32)


def restate_pack(g, r, s=1.0):
    """(v, wire bits, new residual) for gradient g, residual r (None: zeros, no feedback), weight s with g * s exact"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = g * np.float32(s) + (np.float32(0) if r is None else r)
        v = np.asarray(v, np.float32)
        w = rne(v)
        wf = widen(w)
        res = np.where(np.isfinite(wf) & ~np.isnan(v), v - wf, np.float32(0)).astype(np.float32)
    return v, w, res


def same_wire(got, want, v):
    """wire bits equal; where v is NaN the wire is NaN (by isnan, not by payload)"""
    nan = np.isnan(v)
    return np.array_equal(got[~nan], want[~nan]) and bool(np.isnan(widen(got[nan])).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gradients(n, seed, planted=True):
    """normal * exp(8 * normal) -- thirty-odd binades -- with the planted values spread over it (first, last and in between)"""
    rs = np.random.RandomState(seed)
    g = (rs.randn(n) * np.exp(8 * rs.randn(n))).astype(np.float32)
    g[np.abs(g) < 2.0 ** -100] = 0
    if planted and n >= len(PLANTED):
        g[np.linspace(0, n - 1, len(PLANTED)).astype(np.int64)] = PLANTED          # first, last and in between; n = 9: exactly these, in order
    elif planted:
        k = min(n, len(PLANTED) - 2)
        g[:k] = PLANTED[2:2 + k]                                                   # the ties, 3.4e38, the infinities, NaN
    return g


def residuals(g, seed):
    """a plausible carried residual: below half a bfloat16 ulp of g, zero where g is not finite or planted exactly"""
    rs = np.random.RandomState(seed)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (g * (2.0 ** -9) * rs.uniform(-1, 1, len(g))).astype(np.float32)
    r[~np.isfinite(g) | (np.abs(g) > 1e38) | (np.abs(r) < 2.0 ** -120)] = 0
    for p in PLANTED[2:5]:
        r[g == p] = 0                                            # the ties and near-ties stay what they are
    return r


# ---- buffers with guard elements, at a chosen alignment ---------------------------------------------------------------------------
def _addr(buf):
    p = buf.ptr
    return p.value if isinstance(p, ctypes.c_void_p) else int(p)


class Guarded:
    """n elements inside a longer backend buffer: the payload starts 16-byte aligned (+ `skew` elements), GUARD or more elements of a
    fill pattern lie in front of and behind it"""

    def __init__(self, bk, payload, fill, skew=0):
        payload = np.ascontiguousarray(payload)
        self.n, self.dt = len(payload), payload.dtype
        total = self.n + 3 * GUARD + 16
        host = np.full(total, fill, self.dt)
        probe = bk.dev(host)
        it = self.dt.itemsize
        self.off = next(o for o in range(GUARD, GUARD + 16) if (_addr(probe) + o * it) % 16 == 0) + skew
        host[self.off:self.off + self.n] = payload
        self.fill = np.full(1, fill, self.dt)
        # (the interpreter's buffers ARE the numpy array handed in; the device copy has its own address: same residue, both allocators
        # return 16-byte aligned blocks -- asserted)
        self.buf = bk.dev(host) if bk.name != "emul" else probe
        if bk.name == "emul":
            probe.a[...] = host
        assert (_addr(self.buf) + (self.off - skew) * it) % 16 == 0
        self.ptr = ctypes.c_void_p(_addr(self.buf) + self.off * it)

    def get(self):
        return self.buf.get()[self.off:self.off + self.n].copy()

    def guards_intact(self):
        a = self.buf.get()
        f = self.fill.view(np.uint8)
        front, back = a[:self.off].view(np.uint8).reshape(-1, len(f)), a[self.off + self.n:].view(np.uint8).reshape(-1, len(f))
        return bool((front == f).all() and (back == f).all())


def run_pack(bk, g, r, s=1.0, skew=0):
    """-> (wire bits, residual after or None, the buffers) ; asserts the status, that grad is unchanged and that the guards are intact"""
    G = Guarded(bk, g, 7.0, skew)
    R = None if r is None else Guarded(bk, r, 5.0, skew)
    W = Guarded(bk, np.full(len(g), 0x1234, np.uint16), 0xA5A5, skew)
    rc = bk.lib.step_grad_pack16(BF16, G.ptr, None if R is None else R.ptr, W.ptr, len(g), s, bk.stream)
    assert rc == 0, rc
    assert np.array_equal(bits(G.get()), bits(g)) and G.guards_intact(), "grad is read only"
    assert W.guards_intact() and (R is None or R.guards_intact()), "guard elements"
    return W.get(), None if R is None else R.get()


# ---- kernel cases --------------------------------------------------------------------------------------------------------------
def case_pack_bit_exact(bk, golden):
    """step_grad_pack16 at pre_scale = 1 against the restatement: n in {0, 1, 7, 8, 9, 2368, 65536 + 3}, with and without a residual,
    base pointers 16-byte aligned (vector body + scalar tail) and offset by one element (scalar body).  Wire bits equal (NaN by isnan),
    residual bits equal, widen(w) + r' == v bitwise wherever w is finite, grad unchanged, guard elements untouched."""
    for k, n in enumerate(SIZES):
        g = gradients(n, 100 + k)
        for with_res in (True, False):
            r = residuals(g, 200 + k) if with_res else None
            v, want_w, want_r = restate_pack(g, r)
            fin = np.isfinite(widen(want_w))
            assert np.array_equal(bits(widen(want_w)[fin] + want_r[fin]), bits(v[fin])), "the restatement's residual is exact"
            for skew in (0, 1):
                w, r2 = run_pack(bk, g, r, 1.0, skew)
                assert same_wire(w, want_w, v), (n, with_res, skew, "wire")
                if with_res:
                    assert np.array_equal(bits(r2), bits(want_r)), (n, skew, "residual")
                    assert np.array_equal(bits(widen(w)[fin] + r2[fin]), bits(v[fin])), (n, skew, "nothing lost")
    # the planted values, spelled out (n = 9 holds exactly these, in order)
    v, w, r = restate_pack(PLANTED, np.zeros(9, np.float32))
    assert [int(x) for x in w[:8]] == [0x0000, 0x0000, 0x3F80, 0x3F81, 0x3F82, 0x7F80, 0x7F80, 0xFF80]      # (-0 + +0 = +0; tie to even; up; tie to even 1.015625; inf)
    assert r[5] == 0 and r[6] == 0 and r[8] == 0 and r[2] == np.float32(2.0 ** -8) and r[4] == np.float32(-(2.0 ** -8))


def case_pack_weights(bk, golden):
    """pre_scale in {0.5, 4}: bit-exact against the same restatement (the product is exact).  pre_scale = 3 (a tube count): the kernel's own
    v' = widen(w) + r' lies within one float32 ulp of the float64 3 g + r, and w == rne(v')."""
    n = 2368 + 5
    g = gradients(n, 31)
    g[(np.abs(g) > 1e37) & np.isfinite(g)] = 1.0                 # (4 g stays finite where g is; the infinities and NaN stay planted)
    r = residuals(g, 32)
    for s in (0.5, 4.0):
        v, want_w, want_r = restate_pack(g, r, s)
        for skew in (0, 1):
            w, r2 = run_pack(bk, g, r, s, skew)
            assert same_wire(w, want_w, v) and np.array_equal(bits(r2), bits(want_r)), (s, skew)
        v, want_w, _ = restate_pack(g, None, s)
        w, _ = run_pack(bk, g, None, s)
        assert same_wire(w, want_w, v), (s, "no residual")
    fin = np.isfinite(g)
    g3, r3 = g[fin], r[fin]
    w, r2 = run_pack(bk, g3, r3, 3.0)
    v_own = widen(w) + r2                                        # exact: the kernel's v
    ref = 3.0 * g3.astype(np.float64) + r3.astype(np.float64)
    ulp = np.spacing(np.abs(v_own)).astype(np.float64)
    worst = float(np.max(np.abs(v_own.astype(np.float64) - ref) / ulp))
    print("pack at pre_scale = 3 (%s): worst |v' - (3 g + r)| = %.3f ulp" % (bk.name, worst))
    assert worst <= 1.0, worst
    assert np.array_equal(w, rne(v_own))


def case_unpack_all_patterns(bk, golden):
    """step_grad_unpack16 over every 16-bit pattern once (n = 65536): output bits == pattern << 16, NaN payloads included; aligned and
    offset by one element; the wire is read only, guards untouched."""
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for skew in (0, 1):
        W = Guarded(bk, pat, 0xA5A5, skew)
        G = Guarded(bk, np.full(65536, 9.0, np.float32), 7.0, skew)
        assert bk.lib.step_grad_unpack16(BF16, W.ptr, G.ptr, 65536, bk.stream) == 0
        assert np.array_equal(G.get().view(np.uint32), pat.astype(np.uint32) << np.uint32(16)), skew
        assert np.array_equal(W.get(), pat) and W.guards_intact() and G.guards_intact()


def case_feedback_accumulates(bk, golden):
    """What the residual is for: n = 64, constant gradient c = 1 + 2^-10 packed 256 times with the residual carried.  In float64 the sum of
    what went over the wire plus the last residual is 256 c exactly (every intermediate is a multiple of 2^-10: no rounding enters);
    the same loop without a residual sends 1.0 every time and ends short by exactly 0.25."""
    n, c, T = 64, np.float32(1 + 2.0 ** -10), 256
    g = np.full(n, c, np.float32)
    G = Guarded(bk, g, 7.0)
    R = Guarded(bk, np.zeros(n, np.float32), 5.0)
    W = Guarded(bk, np.zeros(n, np.uint16), 0xA5A5)
    total, plain = np.zeros(n, np.float64), np.zeros(n, np.float64)
    for _ in range(T):
        assert bk.lib.step_grad_pack16(BF16, G.ptr, R.ptr, W.ptr, n, 1.0, bk.stream) == 0
        total += widen(W.get()).astype(np.float64)
    assert np.array_equal(total + R.get().astype(np.float64), np.full(n, T * np.float64(c)))
    assert R.guards_intact() and W.guards_intact()
    for _ in range(T):
        assert bk.lib.step_grad_pack16(BF16, G.ptr, None, W.ptr, n, 1.0, bk.stream) == 0
        plain += widen(W.get()).astype(np.float64)
    assert np.array_equal(plain, np.full(n, 256.0)) and np.array_equal(T * np.float64(c) - plain, np.full(n, 0.25))


def case_wire_errors(bk, golden):
    """STEP_F16 / STEP_F32 wire: STEP_E_UNSUPPORTED; n = -1: STEP_E_SHAPE; a NULL wire (or grad) with n = 8: STEP_E_NULL; n = 0 with NULL
    pointers: STEP_OK.  A refused call has written nothing."""
    n = 8
    g = gradients(n, 5, planted=False)
    G, R, W = Guarded(bk, g, 7.0), Guarded(bk, np.full(n, 0.5, np.float32), 5.0), Guarded(bk, np.full(n, 0x1234, np.uint16), 0xA5A5)
    L = bk.lib
    for dt in (F16, F32):
        assert L.step_grad_pack16(dt, G.ptr, R.ptr, W.ptr, n, 1.0, bk.stream) == E_UNSUPPORTED
        assert L.step_grad_unpack16(dt, W.ptr, G.ptr, n, bk.stream) == E_UNSUPPORTED
    assert L.step_grad_pack16(7, G.ptr, R.ptr, W.ptr, n, 1.0, bk.stream) < 0
    assert L.step_grad_pack16(BF16, G.ptr, R.ptr, W.ptr, -1, 1.0, bk.stream) == E_SHAPE
    assert L.step_grad_unpack16(BF16, W.ptr, G.ptr, -1, bk.stream) == E_SHAPE
    assert L.step_grad_pack16(BF16, G.ptr, R.ptr, None, n, 1.0, bk.stream) == E_NULL
    assert L.step_grad_pack16(BF16, None, R.ptr, W.ptr, n, 1.0, bk.stream) == E_NULL
    assert L.step_grad_unpack16(BF16, None, G.ptr, n, bk.stream) == E_NULL
    assert L.step_grad_unpack16(BF16, W.ptr, None, n, bk.stream) == E_NULL
    assert L.step_grad_pack16(BF16, None, None, None, 0, 1.0, bk.stream) == 0
    assert L.step_grad_unpack16(BF16, None, None, 0, bk.stream) == 0
    assert np.array_equal(bits(G.get()), bits(g)) and np.all(R.get() == 0.5) and np.all(W.get() == 0x1234)
    assert G.guards_intact() and R.guards_intact() and W.guards_intact()


def big_pack_unpack(bk, golden):
    """n = 2^22 + 3: one pass of the grid (2048 workgroups x 256 lanes x 8 elements) covers 2^22 elements, the rest is the tail; pack with a
    residual and unpack against the restatement."""
    n = (1 << 22) + 3
    g = gradients(n, 77)
    r = residuals(g, 78)
    v, want_w, want_r = restate_pack(g, r)
    w, r2 = run_pack(bk, g, r)
    assert same_wire(w, want_w, v) and np.array_equal(bits(r2), bits(want_r))
    W, G = Guarded(bk, w, 0xA5A5), Guarded(bk, np.zeros(n, np.float32), 7.0)
    assert bk.lib.step_grad_unpack16(BF16, W.ptr, G.ptr, n, bk.stream) == 0
    assert np.array_equal(G.get().view(np.uint32), w.astype(np.uint32) << np.uint32(16)) and G.guards_intact()


KERNEL_CASES = ["case_pack_bit_exact", "case_pack_weights", "case_unpack_all_patterns", "case_feedback_accumulates", "case_wire_errors"]
KERNEL_GPU_ONLY = ["big_pack_unpack"]


# ---- module cases --------------------------------------------------------------------------------------------------------------
def toy_model(dev):
    """the four-tensor Conv3d + Linear toy of tests/test_dist_gloo.py"""
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv3d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(4 * 2 * 4 * 4, 5))
    return m.to(dev)


def toy_batch(dev, seed=1, n=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 2, 4, 4, generator=g).to(dev), torch.randn(n, 5, generator=g).to(dev)


def torch_restate(g, r):
    """the torch restatement of one pack: (what comes back from a one-rank exchange, the new residual)"""
    v = g + r
    back = v.to(torch.bfloat16).float()
    return back, v - back


def tbits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@contextlib.contextmanager
def one_rank_group(dev):
    """a ONE-rank gloo group (file:// store) for the length of a case.  On "cuda": should this gloo build refuse bfloat16 device tensors, the
    collective of the CASE is staged through a host copy -- on the test's side, the product is not touched -- and the fact is printed."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
        orig = dist.all_reduce
        try:
            if dev != "cpu":
                try:
                    orig(torch.ones(8, dtype=torch.bfloat16, device=dev))
                    torch.cuda.synchronize()
                except RuntimeError as e:
                    print("gloo refuses bfloat16 device tensors (%s): the cases stage the wire through a host copy" % str(e).splitlines()[0])
                    dist.all_reduce = host_staged(orig)
            yield
        finally:
            dist.all_reduce = orig
            dist.destroy_process_group()


def host_staged(all_reduce):
    """TEST ONLY: all_reduce of a device tensor through a host copy (for a gloo build without a bfloat16 device path)"""
    class _Done:
        def wait(self):
            return True

    def staged(t, *a, async_op=False, **kw):
        if not t.is_cuda:
            return all_reduce(t, *a, async_op=async_op, **kw)
        torch.cuda.current_stream(t.device).synchronize()
        h = t.cpu()
        all_reduce(h, *a, **kw)
        t.copy_(h)
        return _Done() if async_op else None
    return staged


def _toy(dev, feedback=True, capturable=False, bucket_bytes=256, reducer=True):
    """-> (model, FlatSGD(momentum 0), GradWire, BucketedReducer or None, raw): `raw` receives every parameter's gradient as autograd
    leaves it, from a post-accumulate hook registered AHEAD of the reducer's (hooks run in registration order) -- the gradient of this very
    backward pass, before its bucket is exchanged in place"""
    from step_amd import dist as D
    from step_amd.optim import FlatSGD
    model = toy_model(dev)
    opt = FlatSGD(model.parameters(), lr=2.0 ** -7, momentum=0, capturable=capturable)
    raw = torch.zeros_like(opt.flat_grad)
    def keep(o, n):
        def hook(q):
            raw[o:o + n].copy_(q.grad.reshape(-1))
        return hook
    for _, p, o, n in opt._entries:
        p.register_post_accumulate_grad_hook(keep(o, n))
    wire = D.GradWire(opt, error_feedback=feedback)
    red = D.BucketedReducer(opt, bucket_bytes=bucket_bytes, single_rank=True, wire=wire) if reducer else None
    return model, opt, wire, red, raw


def _backward(model, opt, x, y, red=None, scaler=None):
    opt.zero_grad()
    if red is not None:
        red.begin()
    loss = ((model(x) - y) ** 2).mean()
    (loss if scaler is None else scaler.scale_loss(loss)).backward()
    return red.finish() if red is not None else 1.0


def case_reducer_two_passes(dev, golden):
    """Two successive backward passes through BucketedReducer(wire=GradWire(opt)), bucket_bytes = 256 (several buckets): after each pass
    flat_grad and wire.residual equal the torch restatement bit for bit -- (g + r).to(bfloat16).float() and g + r - that -- the residual
    of pass one being used in pass two; the wire registered itself with the optimizer."""
    with one_rank_group(dev):
        model, opt, wire, red, raw = _toy(dev)
        assert red.active and len(red.buckets) >= 3 and opt.grad_wire is wire
        assert wire.wire.dtype == torch.bfloat16 and wire.wire.numel() == opt.numel
        assert wire.residual.dtype == torch.float32 and wire.residual.numel() == opt.numel and not wire.residual.any()
        r = torch.zeros_like(raw)
        for k in range(2):
            x, y = toy_batch(dev, seed=10 + k)
            assert _backward(model, opt, x, y, red) == 1.0
            back, r = torch_restate(raw.clone(), r)
            assert float(raw.abs().max()) > 0 and float(r.abs().max()) > 0
            assert np.array_equal(tbits(opt.flat_grad), tbits(back)), k
            assert np.array_equal(tbits(wire.residual), tbits(r)), k
            assert np.array_equal(tbits(wire.wire.float()), tbits(back)), k
        red.close()


def case_allreduce_flat_chunks(dev, golden):
    """allreduce_flat(flat, wire=..., single_rank=True) with chunk_bytes = 70 (35 wire elements: does not divide the arena, chunks start off
    the 16-byte grid) gives the bits of one shot; a tensor that is not the wire's arena is refused -- also where the exchange is inactive;
    one rank without single_rank: nothing happens."""
    from step_amd import dist as D
    with one_rank_group(dev):
        model, opt, wire, _, _ = _toy(dev, reducer=False)
        x, y = toy_batch(dev, seed=3)
        _backward(model, opt, x, y)
        g = opt.flat_grad.clone()
        back, r = torch_restate(g, torch.zeros_like(g))
        assert opt.numel % 35 != 0
        for chunk in (512 << 20, 70):
            opt.flat_grad.copy_(g)
            wire.residual.zero_()
            assert D.allreduce_flat(opt.flat_grad, chunk_bytes=chunk, wire=wire, single_rank=True) == 1.0
            assert np.array_equal(tbits(opt.flat_grad), tbits(back)) and np.array_equal(tbits(wire.residual), tbits(r)), chunk
        for single in (True, False):
            try:
                D.allreduce_flat(opt.flat_grad.clone(), wire=wire, single_rank=single)
            except ValueError:
                continue
            raise AssertionError("allreduce_flat accepted a tensor that is not the wire's arena")
        opt.flat_grad.copy_(g)
        wire.residual.zero_()
        assert D.allreduce_flat(opt.flat_grad, wire=wire) == 1.0
        assert np.array_equal(tbits(opt.flat_grad), tbits(g)) and not wire.residual.any()


def case_wire_and_scaler(dev, golden):
    """opt.step(scaler=LossScaler(...)) with a feedback wire raises RuntimeError.  A wire WITHOUT feedback works with the scaler: an inf
    planted in one gradient travels through the exchange, the scaler's found_inf path skips the step (step count and parameters
    unchanged), the scale halves; the next clean step counts."""
    from step_amd import dist as D
    from step_amd.optim import LossScaler
    with one_rank_group(dev):
        scaler = LossScaler(torch.device(dev), init_scale=2.0 ** 10)
        x, y = toy_batch(dev, seed=4)
        model, opt, wire, _, _ = _toy(dev, feedback=True, capturable=True, reducer=False)
        _backward(model, opt, x, y, scaler=scaler)
        p0 = opt.flat_param.clone()
        try:
            opt.step(scaler=scaler, zero_grad=True)
        except RuntimeError as e:
            assert "feedback" in str(e), e
        else:
            raise AssertionError("a feedback wire was accepted together with a LossScaler")
        assert torch.equal(opt.flat_param, p0) and opt.step_count == 0 and scaler.scale == 2.0 ** 10
        model, opt, wire, _, _ = _toy(dev, feedback=False, capturable=True, reducer=False)
        assert wire.residual is None
        p0 = opt.flat_param.clone()
        _backward(model, opt, x, y, scaler=scaler)
        opt.flat_grad[3] = float("inf")
        f = D.allreduce_flat(opt.flat_grad, wire=wire, single_rank=True)
        assert bool(torch.isinf(opt.flat_grad[3])) and bool(torch.isfinite(opt.flat_grad[4:]).all())
        opt.step(scaler=scaler, grad_scale=f, zero_grad=True)
        assert opt.step_count == 0 and torch.equal(opt.flat_param, p0) and scaler.scale == 2.0 ** 9
        _backward(model, opt, x, y, scaler=scaler)
        f = D.allreduce_flat(opt.flat_grad, wire=wire, single_rank=True)
        opt.step(scaler=scaler, grad_scale=f, zero_grad=True)
        assert opt.step_count == 1 and not torch.equal(opt.flat_param, p0) and scaler.scale == 2.0 ** 9


def case_wire_state_dict(dev, golden):
    """state_dict() carries dtype, the feedback flag and a copy of the residual; loaded into a fresh wire it reproduces the NEXT step's
    wire bits and residual; loaded without the residual the residual restarts at zero (documented as harmless); a dict of another kind of
    wire is refused.  (Hand-made gradients: the same arena values go through both wires.)"""
    from step_amd import dist as D
    with one_rank_group(dev):
        _, opt, wire, _, _ = _toy(dev, reducer=False)
        gen = torch.Generator().manual_seed(8)
        ga, gb = (torch.randn(opt.numel, generator=gen) * torch.exp(2 * torch.randn(opt.numel, generator=gen))).to(dev), torch.randn(opt.numel, generator=gen).to(dev)
        opt.flat_grad.copy_(ga)
        D.allreduce_flat(opt.flat_grad, wire=wire, single_rank=True)
        sd = wire.state_dict()
        assert sd["dtype"] == "bf16" and sd["error_feedback"] is True and torch.equal(sd["residual"], wire.residual) and wire.residual.any()
        assert sd["residual"].data_ptr() != wire.residual.data_ptr()
        opt.flat_grad.copy_(gb)
        D.allreduce_flat(opt.flat_grad, wire=wire, single_rank=True)
        want_w, want_r = wire.wire.clone(), wire.residual.clone()
        wire2 = D.GradWire(opt)
        assert opt.grad_wire is wire2
        wire2.load_state_dict(sd)
        opt.flat_grad.copy_(gb)
        D.allreduce_flat(opt.flat_grad, wire=wire2, single_rank=True)
        assert torch.equal(wire2.wire.view(torch.int16), want_w.view(torch.int16)) and np.array_equal(tbits(wire2.residual), tbits(want_r))
        wire2.load_state_dict({"dtype": "bf16", "error_feedback": True, "residual": None})
        assert not wire2.residual.any()
        plain = D.GradWire(opt, error_feedback=False)
        assert plain.state_dict() == {"dtype": "bf16", "error_feedback": False, "residual": None}
        try:
            plain.load_state_dict(sd)
        except ValueError:
            pass
        else:
            raise AssertionError("a feedback checkpoint was loaded into a wire without feedback")


def case_wire_inactive(dev, golden):
    """With no process group a BucketedReducer(wire=...) leaves flat_grad bit-identical to a run without a wire (the gradient as autograd
    left it): nothing is packed, the residual and the wire arena stay zero; allreduce_flat likewise."""
    import torch.distributed as dist
    from step_amd import dist as D
    assert not dist.is_initialized()
    x, y = toy_batch(dev, seed=7)
    model, opt, wire, red, raw = _toy(dev)
    assert not red.active
    assert _backward(model, opt, x, y, red) == 1.0
    assert float(raw.abs().max()) > 0 and np.array_equal(tbits(opt.flat_grad), tbits(raw))
    assert not wire.residual.any() and not wire.wire.view(torch.int16).any()
    assert D.allreduce_flat(opt.flat_grad, wire=wire, single_rank=True) == 1.0
    assert np.array_equal(tbits(opt.flat_grad), tbits(raw)) and not wire.residual.any()
    red.close()


MODULE_CASES = ["case_reducer_two_passes", "case_allreduce_flat_chunks", "case_wire_and_scaler", "case_wire_state_dict", "case_wire_inactive"]
