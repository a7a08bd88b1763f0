"""Cases for step_pool_then_conv_forward (step_amd/csrc/pool.hip: pool333_then_pw_kernel, option pool_then_conv): an Inception block's
3x3x3 / 1 TF-SAME max pool and the pointwise conv of the pooled tensor as ONE launch that never writes the pooled tensor.  Driven on the
host interpreter by tests/test_emul_poolpw.py and on the real library by tests/test_gpu_poolpw.py.

Every kernel case runs under pool_then_conv = 2 (wherever eligible: the interpreter's maps are far below the workgroup count the default
rule asks for), writes into a channel slice between guard channels and demands (a) np.array_equal against step_maxpool3d_tf followed by
step_conv_forward, (b) untouched guard channels and (c) the project's tolerance against ref_conv(R.maxpool_tf(x))."""
import ctypes

import numpy as np
import torch

from oracle import i3d_ref as R
from step_amd import _capi
from tests.kernel_cases import BF16, F16, F32, NP_DT, cl, decode, encode, pack_weight, quantize, ref_conv, tol, uncl

# name -> (dtype, (N, D, H, W), Cin, Cout, channels of the input buffer, first channel of the slice)
SHAPES = {
    "bf16_3b_2x3x28x28_192x32": (BF16, (2, 3, 28, 28), 192, 32, 192, 0),      # 3b: several tiles, both D edges and an interior plane
    "f16_3c_1x5x28x28_256x64": (F16, (1, 5, 28, 28), 256, 64, 256, 0),        # 3c: two channel blocks, an odd D
    "bf16_1x1x28x28_32x8": (BF16, (1, 1, 28, 28), 32, 8, 32, 0),              # both D pads in one window, one chunk, a partial channel block
    "bf16_slice_1x2x9x11_40x24": (BF16, (1, 2, 9, 11), 40, 24, 56, 8),        # [..., 8:48] of 56 channels: one partial tile, a 99-pixel tail group, a partial last chunk
    "f16_1x4x25x25_64x40": (F16, (1, 4, 25, 25), 64, 40, 64, 0),              # ragged 13 / 12 tiles
    "f16_1x1x50x50_32x32": (F16, (1, 1, 50, 50), 32, 32, 32, 0),              # 4 x 4 tiles
}
KERNEL_CASES = ["case_poolpw_" + k for k in SHAPES] + ["case_poolpw_negative_input", "case_poolpw_nonfinite", "case_poolpw_refusals",
                                                       "case_poolpw_mixed_block"]
KERNEL_GPU_ONLY = ["case_poolpw_default_rule_c2_maps"]


def _desc(dt, shape, Cin, Cout, xcs, xoff, ycs, yoff, **kw):
    N, D, H, W = shape
    f = dict(dtype=dt, N=N, D=D, H=H, W=W, Cin=Cin, Cout=Cout, kd=1, kh=1, kw=1, x_cstride=xcs, x_coff=xoff, y_cstride=ycs, y_coff=yoff,
             res_cstride=0, res_coff=0, relu=1, split=0, y2_cstride=0, y2_coff=0)
    f.update(kw)
    return _capi.ConvDesc(**f)


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a                 # (fp16 buffers are numpy floats: compare NaNs by pattern)


class _Layer:
    """one pool + pointwise layer: the input (a channel slice of a buffer whose other channels hold 77), weights, affine"""

    def __init__(self, bk, dt, shape, Cin, Cout, cbuf, coff, seed, x=None):
        rs = np.random.RandomState(seed)
        N, D, H, W = shape
        self.bk, self.dt, self.shape, self.Cin, self.Cout, self.cbuf, self.coff = bk, dt, shape, Cin, Cout, cbuf, coff
        self.x = rs.randn(N, Cin, D, H, W).astype(np.float32) if x is None else x
        buf = np.full((N, D, H, W, cbuf), 77, np.float32)
        buf[..., coff:coff + Cin] = cl(self.x)
        self.xe = bk.dev(encode(buf, dt))
        self.w = (rs.randn(Cout, Cin, 1, 1, 1) / np.sqrt(Cin)).astype(np.float32)
        self.sc, self.sh = (1 + 0.1 * rs.randn(Cout)).astype(np.float32), (0.2 * rs.randn(Cout)).astype(np.float32)
        self.wp, self.dsc, self.dsh = pack_weight(bk, self.w, dt), bk.dev(self.sc), bk.dev(self.sh)
        self.ctot = 8 + Cout + 8

    def two_launches(self):
        bk, dt, (N, D, H, W), Cin = self.bk, self.dt, self.shape, self.Cin
        py = bk.dev(np.zeros((N, D, H, W, Cin), NP_DT[dt]))
        y = bk.dev(np.zeros((N, D, H, W, self.ctot), NP_DT[dt]))
        d = _desc(dt, self.shape, Cin, self.Cout, Cin, 0, self.ctot, 8)
        assert bk.lib.step_maxpool3d_tf(dt, self.xe.ptr, N, D, H, W, Cin, self.cbuf, self.coff, 3, 3, 3, 1, 1, 1, py.ptr, Cin, 0, bk.stream) == 0
        assert bk.lib.step_conv_forward(ctypes.byref(d), py.ptr, self.wp.ptr, self.dsc.ptr, self.dsh.ptr, None, y.ptr, None, bk.stream) == 0
        return y.get()

    def fused(self, **opts):
        bk, dt, (N, D, H, W) = self.bk, self.dt, self.shape
        y = bk.dev(np.zeros((N, D, H, W, self.ctot), NP_DT[dt]))
        d = _desc(dt, self.shape, self.Cin, self.Cout, self.cbuf, self.coff, self.ctot, 8)
        with _capi.options(bk.lib, **opts):
            nbc = bk.lib.step_pool_then_conv_plan(ctypes.byref(d))
            assert nbc == (self.Cout + 31) // 32, nbc
            assert bk.lib.step_pool_then_conv_forward(dt, self.xe.ptr, N, D, H, W, self.cbuf, self.coff, ctypes.byref(d), self.wp.ptr, self.dsc.ptr,
                                                      self.dsh.ptr, y.ptr, bk.stream) == 0
        return y.get()

    def reference(self):
        p = R.maxpool_tf(torch.from_numpy(quantize(self.x, self.dt)), (3, 3, 3), (1, 1, 1)).numpy()
        return ref_conv(p, self.w, self.sc, self.sh, self.dt)

    def check(self, got, sep):
        assert np.array_equal(_bits(got), _bits(sep)), "the fused launch differs from pool + conv"
        y = decode(got, self.dt)
        assert not y[..., :8].any() and not y[..., self.ctot - 8:].any()      # guard channels untouched
        ref = self.reference()
        err = np.abs(uncl(y[..., 8:8 + self.Cout]) - ref).max() / np.abs(ref).max()
        assert err < tol(self.dt), err


def _case(name, seed):
    def case(bk, golden):
        dt, shape, Cin, Cout, cbuf, coff = SHAPES[name]
        L = _Layer(bk, dt, shape, Cin, Cout, cbuf, coff, seed)
        L.check(L.fused(pool_then_conv=2), L.two_launches())
    case.__name__ = "case_poolpw_" + name
    case.__doc__ = "pool + pointwise conv in one launch %s against the two launches and ref_conv(maxpool_tf)" % (SHAPES[name],)
    return case


for _i, _name in enumerate(SHAPES):
    globals()["case_poolpw_" + _name] = _case(_name, 211 + _i)


def case_poolpw_negative_input(bk, golden):
    """x = -|randn| - 1: every window at a border of the map or the clip must return the explicit TF pad's 0 -- not its largest negative
    element -- before the GEMM (and the interior its negative maximum)."""
    rs = np.random.RandomState(31)
    shape = (1, 3, 17, 15)
    x = (-np.abs(rs.randn(1, 48, 3, 17, 15)) - 1).astype(np.float32)
    L = _Layer(bk, BF16, shape, 48, 16, 48, 0, 32, x=x)
    p = R.maxpool_tf(torch.from_numpy(quantize(x, BF16)), (3, 3, 3), (1, 1, 1)).numpy()
    assert (p[:, :, 0] == 0).all() and (p[:, :, :, 0] == 0).all() and (p[:, :, :, :, -1] == 0).all() and (p[:, :, 1, 1:-1, 1:-1] < 0).all()
    L.check(L.fused(pool_then_conv=2), L.two_launches())


def case_poolpw_nonfinite(bk, golden):
    """NaN of both signs, +inf and -inf in x (tests/nonfinite_cases.plant): the one-launch form gives the bits of the two launches, NaN for
    NaN (the non-finite contract of include/step_amd.h), in both storage types."""
    from tests.nonfinite_cases import cls, plant
    rs = np.random.RandomState(33)
    for dt in (BF16, F16):
        x, _ = plant(rs.randn(1, 40, 3, 16, 15).astype(np.float32), dt)
        L = _Layer(bk, dt, (1, 3, 16, 15), 40, 24, 40, 0, 34, x=x)
        got, sep = L.fused(pool_then_conv=2), L.two_launches()
        assert np.array_equal(_bits(got), _bits(sep)), dt
        c = np.bincount(cls(decode(got, dt)[..., 8:32]).ravel(), minlength=4)
        assert c[3] > 0 and c[0] > 0, c.tolist()                               # NaNs came through and finite values stayed


def case_poolpw_refusals(bk, golden):
    """What the form does not cover is refused before any launch -- the library returns STEP_E_UNSUPPORTED / STEP_E_ALIGN and plans 0, the
    wrapper returns None and leaves no ops.PROFILE record: fp32, Cin = 12, a [..., 4:] slice off the 16-byte grid, Cout = 136, Cin = 264.
    N = 0 is accepted.  The option's default is the rule (1), which leaves maps of a few tiles to the two launches."""
    from step_amd import ops
    from tests.emul.patch import emulated_kernels
    import contextlib
    shape = (1, 2, 9, 11)
    N, D, H, W = shape
    xe = bk.dev(np.zeros((N, D, H, W, 272), np.float32))
    wp, y = bk.dev(np.zeros(1 << 16, np.float32)), bk.dev(np.zeros((N, D, H, W, 272), np.float32))
    with _capi.options(bk.lib, pool_then_conv=2):
        for dt, Cin, Cout, xcs, want in ((F32, 32, 32, 32, (-4,)), (BF16, 12, 32, 16, (-4, -5)), (BF16, 32, 136, 32, (-4,)), (BF16, 264, 32, 264, (-4,))):
            d = _desc(dt, shape, Cin, Cout, xcs, 0, 144, 0)
            assert bk.lib.step_pool_then_conv_plan(ctypes.byref(d)) == 0, (dt, Cin, Cout)
            assert bk.lib.step_pool_then_conv_forward(dt, xe.ptr, N, D, H, W, xcs, 0, ctypes.byref(d), wp.ptr, None, None, y.ptr, bk.stream) in want, (dt, Cin, Cout)
        d = _desc(BF16, shape, 32, 32, 40, 0, 32, 0)
        off = ctypes.c_void_p(ctypes.cast(xe.ptr, ctypes.c_void_p).value + 8)          # the address of a [..., 4:36] slice of 40 bf16 channels
        assert bk.lib.step_pool_then_conv_forward(BF16, off, N, D, H, W, 40, 0, ctypes.byref(d), wp.ptr, None, None, y.ptr, bk.stream) == -5
        d0 = _desc(BF16, (0, 2, 9, 11), 32, 32, 32, 0, 32, 0)
        assert bk.lib.step_pool_then_conv_forward(BF16, None, 0, 2, 9, 11, 32, 0, ctypes.byref(d0), None, None, None, None, bk.stream) == 0
        dsplit = _desc(BF16, shape, 32, 32, 32, 0, 32, 0, split=16, y2_cstride=16)
        assert bk.lib.step_pool_then_conv_plan(ctypes.byref(dsplit)) == 0
    ok = _desc(BF16, shape, 32, 32, 32, 0, 32, 0)
    v = ctypes.c_int(-1)
    assert bk.lib.step_get_option(_capi.OPTION_IDS["pool_then_conv"], ctypes.byref(v)) == 0 and v.value == 1
    assert bk.lib.step_pool_then_conv_plan(ctypes.byref(ok)) == 0                        # (4 workgroups: below the default rule)
    assert bk.lib.step_pool_then_conv_forward(BF16, xe.ptr, N, D, H, W, 32, 0, ctypes.byref(ok), wp.ptr, None, None, y.ptr, bk.stream) == -4
    with _capi.options(bk.lib, pool_then_conv=0):
        assert bk.lib.step_pool_then_conv_plan(ctypes.byref(ok)) == 0
    assert bk.lib.step_set_option(_capi.OPTION_IDS["pool_then_conv"], 3) != 0
    assert not y.get().any()                                                         # nothing was launched
    # ---- the wrapper: None and no record
    dev = "cuda" if bk.name == "gfx950" else "cpu"
    bf, t = torch.bfloat16, (lambda s, dt_: torch.zeros(s, dtype=dt_, device=dev))
    w = t((1 << 16,), bf)
    calls = [lambda: ops.pool_then_conv_forward(t((1, 2, 9, 11, 32), torch.float32), t((1 << 16,), torch.float32), 32, None, None, True, t((1, 2, 9, 11, 32), torch.float32)),
             lambda: ops.pool_then_conv_forward(t((1, 2, 9, 11, 12), bf), w, 32, None, None, True, t((1, 2, 9, 11, 32), bf)),
             lambda: ops.pool_then_conv_forward(t((1, 2, 9, 11, 40), bf)[..., 4:36], w, 32, None, None, True, t((1, 2, 9, 11, 32), bf)),
             lambda: ops.pool_then_conv_forward(t((1, 2, 9, 11, 32), bf), w, 136, None, None, True, t((1, 2, 9, 11, 136), bf)),
             lambda: ops.pool_then_conv_forward(t((1, 2, 9, 11, 264), bf), w, 32, None, None, True, t((1, 2, 9, 11, 32), bf))]
    with (emulated_kernels() if dev == "cpu" else contextlib.nullcontext()):
        with _capi.options(bk.lib, pool_then_conv=2):
            try:
                ops.PROFILE, ops.PROFILE_LIMIT = [], 1 << 30
                for k, call in enumerate(calls):
                    assert call() is None, k
                    assert ops.PROFILE == [], (k, ops.PROFILE)
                out = t((1, 2, 9, 11, 32), bf)
                assert ops.pool_then_conv_forward(t((1, 2, 9, 11, 32), bf), w, 32, None, None, True, out) is out
                assert len(ops.PROFILE) == 1 and ops.PROFILE[0][0].startswith("void step::pool333_then_pw_kernel<step::bf16_t, 1>("), ops.PROFILE
                pix = 2 * 9 * 11
                assert ops.PROFILE[0][1] == 2.0 * pix * 32 * 32 and ops.PROFILE[0][2] == (pix * 64 + 32 * 32) * 2
            finally:
                ops.PROFILE, ops.PROFILE_LIMIT = None, None


def case_poolpw_mixed_block(bk, golden):
    """Mixed_3b's and Mixed_3c's channel tables.  (a) Executed on a (1, 2, 28, 28) map under pool_then_conv = 2, the pool standing alone as
    on C2's maps (on a map this small the library would carry 3c's pool in the triple's grid: backbone.POOL_WITH_POINTWISE off): the
    inference forward with backbone.POOL_THEN_POINTWISE on equals the forward with it off bit for bit, records the one-launch kernel once,
    no pool, and one launch fewer wherever branch_3's conv was a launch of its own (the same number where it rode in the grouped launch,
    which then carries its two-member name).  (b) Recorded without launching (ops.PROFILE_LIMIT = 0) on C2's own (8, 16, 28, 28) maps
    under the default options and switches: 3b is one launch fewer (its pool and its 192 -> 32 conv were two), 3c keeps its count and its
    grouped record changes from conv_tap_group_pw_kernel... to the two-member name (the 256 -> 64 conv left the group)."""
    import contextlib
    from step_amd import backbone, ops
    from tests.emul.patch import emulated_kernels
    from tests.module_cases import fill
    dev = "cuda" if bk.name == "gfx950" else "cpu"
    grp = lambda ns: [n for n in ns if "conv_tap_group" in n]

    def forward(m, x, on, limit):
        try:
            backbone.POOL_THEN_POINTWISE = on
            ops.PROFILE, ops.PROFILE_LIMIT = [], limit
            y = m(x).clone()
            return y, [r[0] for r in ops.PROFILE]
        finally:
            backbone.POOL_THEN_POINTWISE = True
            ops.PROFILE, ops.PROFILE_LIMIT = None, None

    with (emulated_kernels() if dev == "cpu" else contextlib.nullcontext()), torch.no_grad():
        assert backbone.POOL_THEN_POINTWISE and backbone.POOL_WITH_POINTWISE
        for blk, dt in (("3b", torch.bfloat16), ("3c", torch.float16)):
            cin, oc = backbone.MIXED_CFG[blk]
            m = fill(backbone.Mixed(cin, oc), "golden.poolpw.%s." % blk).to(dev).eval()
            # ---- (a)
            x = R.fill_tensor("golden.poolpw.x" + blk, (1, 2, 28, 28, cin), "feat").to(dev).to(dt)
            outs, names = {}, {}
            try:
                backbone.POOL_WITH_POINTWISE = False
                with _capi.options(bk.lib, pool_then_conv=2):
                    for on in (True, False):
                        outs[on], names[on] = forward(m, x, on, 1 << 30)
            finally:
                backbone.POOL_WITH_POINTWISE = True
            assert torch.equal(outs[True], outs[False]), blk
            assert bool(torch.isfinite(outs[True].float()).all()) and float(outs[True].float().abs().max()) > 0
            assert sum("pool333_then_pw_kernel" in n for n in names[True]) == 1 and not any("pool333_then_pw_kernel" in n for n in names[False]), names
            assert not any("maxpool" in n for n in names[True]) and sum("maxpool_sep_kernel" in n for n in names[False]) == 1, names
            rode = any("_pw_kernel" in n for n in grp(names[False]))
            assert len(names[True]) == len(names[False]) - (0 if rode else 1), names
            assert not any("_pw_kernel" in n for n in grp(names[True])), names
            # ---- (b)
            xb = torch.empty((8, 16, 28, 28, cin), dtype=torch.bfloat16, device=dev)
            _, on_ = forward(m, xb, True, 0)
            _, off = forward(m, xb, False, 0)
            assert sum("pool333_then_pw_kernel" in n for n in on_) == 1 and not any("maxpool" in n for n in on_), on_
            assert len(grp(on_)) == 1 and len(grp(off)) == 1 and "_pw_kernel" not in grp(on_)[0], (on_, off)
            if blk == "3b":
                assert len(on_) == len(off) - 1 and "_pw_kernel" not in grp(off)[0], (on_, off)
            else:
                assert len(on_) == len(off) and "conv_tap_group_pw_kernel" in grp(off)[0], (on_, off)
                assert grp(on_)[0] == grp(off)[0].replace("conv_tap_group_pw_kernel", "conv_tap_group_kernel"), (on_, off)


def case_poolpw_default_rule_c2_maps(bk, golden):
    """C2's own layers (8 clips, 16 x 28 x 28 maps: Mixed_3b 192 -> 32, Mixed_3c 256 -> 64): step_pool_then_conv_plan takes the form under the
    DEFAULT option value; one clip of each equals the separate calls."""
    for dt, Cin, Cout, seed in ((BF16, 192, 32, 5), (BF16, 256, 64, 6)):
        d = _desc(dt, (8, 16, 28, 28), Cin, Cout, Cin, 0, Cout, 0)
        assert bk.lib.step_pool_then_conv_plan(ctypes.byref(d)) == (Cout + 31) // 32
        L = _Layer(bk, dt, (1, 16, 28, 28), Cin, Cout, Cin, 0, seed)
        L.check(L.fused(pool_then_conv=2), L.two_launches())
