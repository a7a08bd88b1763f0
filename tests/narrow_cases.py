"""Cases for the pixel-split form of step_conv_forward_group's narrow members (step_amd/csrc/conv_tap_narrow.h, option
conv_group_narrow), driven on the host interpreter by tests/test_emul_narrow.py and on the real library by tests/test_gpu_narrow.py.

Every case launches a wide 3x3x3 member (an Inception block's branch_1 shape) and a narrow one (branch_2: Cin <= 32, Cout <= 96) --
with or without the block's pointwise third member -- as ONE call, outputs = channel slices of one buffer between guard channels, and
demands np.array_equal against (a) one step_conv_forward per item and (b) the same grouped call under conv_group_narrow = 0 (the
partner's instantiation for every member), under the default and the `throughput` planner profile; the narrow member is also held to
ref_conv with the project's tolerance (image borders and ragged boxes included).  conv_group_narrow = 2 takes the form wherever it is
eligible: the interpreter's maps are far below the tile count the default rule asks for."""
import ctypes

import numpy as np

from step_amd import _capi
from tests.kernel_cases import BF16, F16, NP_DT, cl, decode, encode, pack_weight, ref_conv, tol, uncl

# The planner sends a Cin < 64 conv to the pipelined kernel (and so into a group) from 32 tiles of 256 pixels on, and takes general
# boxes where they save tiles against the power-of-two shapes: every map below does both for every member.
MAP28 = (3, 4, 28, 28)                                       # 42 boxes of 4 x 4 x 14 -> 21 of 4 x 4 x 28 (column runs of 16)
MAP14 = (5, 8, 14, 14)                                       # 35 boxes of 8 x 2 x 14 -> 20 of 2 x 14 x 14
RAG25 = (1, 11, 25, 25)                                      # ragged in every axis: 25-wide rows (linear row walk), D = 11

# name -> (dtype, (N, D, H, W), wide (Cin, Cout), narrow (Cin, Cout), pointwise (Cin, Cout) or None)
CONFIGS = {
    "bf16_28_16x32_pw": (BF16, MAP28, (96, 128), (16, 32), (192, 32)),        # Mixed_3b
    "bf16_28_32x96": (BF16, MAP28, (64, 192), (32, 96), None),                # Mixed_3c
    "f16_28_32x40": (F16, MAP28, (64, 64), (32, 40), None),
    "f16_14_16x48_pw": (F16, MAP14, (96, 208), (16, 48), (128, 64)),          # Mixed_4b
    "bf16_14_24x64": (BF16, MAP14, (64, 64), (24, 64), None),                 # Mixed_4c
    "bf16_14_32x64_pw": (BF16, MAP14, (64, 72), (32, 64), (136, 72)),         # Mixed_4e
    "f16_14_32x96": (F16, MAP14, (64, 64), (32, 96), None),
    "bf16_r25_8x24_pw": (BF16, RAG25, (64, 64), (8, 24), (128, 40)),
    "f16_r25_24x64": (F16, RAG25, (64, 64), (24, 64), None),
    "f16_r25_16x32": (F16, RAG25, (64, 64), (16, 32), None),
    "bf16_r25_32x40": (BF16, RAG25, (64, 64), (32, 40), None),
}
KERNEL_CASES = ["case_narrow_" + k for k in CONFIGS] + ["case_narrow_kernel_names"]
KERNEL_GPU_ONLY = ["case_narrow_default_rule_c2_maps"]


def _ptr(b):
    return ctypes.cast(b.ptr, ctypes.c_void_p).value


class _Group:
    """the items of one grouped call: inputs, weights, affine tables and the item array (order: wide, narrow[, pointwise])"""

    def __init__(self, bk, dt, shape, wide, narrow, pw, seed):
        rs = np.random.RandomState(seed)
        N, D, H, W = shape
        self.bk, self.dt, self.shape = bk, dt, shape
        (ci0, co0), (ci1, co1) = wide, narrow
        self.t = rs.randn(N, ci0 + ci1, D, H, W).astype(np.float32)           # the shared bottleneck buffer: member k reads its slice
        self.te = bk.dev(encode(cl(self.t), dt))
        self.specs = [(ci0, co0, 3, self.te, ci0 + ci1, 0), (ci1, co1, 3, self.te, ci0 + ci1, ci0)]
        self.src = [self.t[:, :ci0], self.t[:, ci0:]]
        if pw:
            self.pl = rs.randn(N, pw[0], D, H, W).astype(np.float32)          # the pooled tensor: another buffer
            self.pe = bk.dev(encode(cl(self.pl), dt))
            self.specs.append((pw[0], pw[1], 1, self.pe, pw[0], 0))
            self.src.append(self.pl)
        self.ws = [(rs.randn(co, ci, k, k, k) / np.sqrt(ci * k ** 3)).astype(np.float32) for ci, co, k, _, _, _ in self.specs]
        self.aff = [((1 + 0.1 * rs.randn(co)).astype(np.float32), (0.2 * rs.randn(co)).astype(np.float32)) for _, co, _, _, _, _ in self.specs]
        self.wp = [pack_weight(bk, w, dt) for w in self.ws]
        self.sc = [(bk.dev(a), bk.dev(b)) for a, b in self.aff]
        self.ctot = 8 + sum(s[1] for s in self.specs) + 8
        self.n = len(self.specs)

    def items(self, yb):
        items, keep, yoff = (_capi.ConvItem * self.n)(), [], 8
        N, D, H, W = self.shape
        for k, (ci, co, kk, xb, xcs, xoff) in enumerate(self.specs):
            d = _capi.ConvDesc(dtype=self.dt, N=N, D=D, H=H, W=W, Cin=ci, Cout=co, kd=kk, kh=kk, kw=kk, x_cstride=xcs, x_coff=xoff,
                               y_cstride=self.ctot, y_coff=yoff, res_cstride=0, res_coff=0, relu=1, split=0, y2_cstride=0, y2_coff=0)
            keep.append(d)
            it = items[k]
            it.desc = ctypes.pointer(d)
            it.x, it.w_packed, it.scale, it.shift, it.res, it.y = (_ptr(xb), _ptr(self.wp[k]), _ptr(self.sc[k][0]), _ptr(self.sc[k][1]), None, _ptr(yb))
            yoff += co
        return items, keep

    def run(self, grouped, **opts):
        """-> (output buffer, kernel name the planner reports for the grouped call under these options)"""
        bk = self.bk
        yb = bk.dev(np.zeros(self.shape + (self.ctot,), NP_DT[self.dt]))
        items, keep = self.items(yb)
        buf = ctypes.create_string_buffer(256)
        with _capi.options(bk.lib, **opts):
            assert bk.lib.step_conv_group_kernel_name(items, self.n, buf, 256) == 0
            if grouped:
                assert bk.lib.step_conv_forward_group(items, self.n, bk.stream) == 0
            else:
                for k in range(self.n):
                    it = items[k]
                    assert bk.lib.step_conv_forward(it.desc, it.x, it.w_packed, it.scale, it.shift, None, it.y, None, bk.stream) == 0
        return yb.get(), buf.value

    def check_against_reference(self, out):
        y = decode(out, self.dt)
        assert not y[..., :8].any() and not y[..., self.ctot - 8:].any()      # guard channels untouched
        lo = 8
        for k, (ci, co, kk, _, _, _) in enumerate(self.specs):
            ref = ref_conv(self.src[k], self.ws[k], self.aff[k][0], self.aff[k][1], self.dt)
            got = uncl(y[..., lo:lo + co])
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err < tol(self.dt), (k, ci, co, err)
            lo += co


def _case(cfg, seed):
    def case(bk, golden):
        dt, shape, wide, narrow, pw = CONFIGS[cfg]
        g = _Group(bk, dt, shape, wide, narrow, pw, seed)
        sep, _ = g.run(False)
        new, name_new = g.run(True, conv_group_narrow=2)
        old, name_old = g.run(True, conv_group_narrow=0)
        thr, name_thr = g.run(True, conv_group_narrow=2, throughput=1)
        # the form really ran, in both planner profiles; the pointwise member rides exactly where it rides today
        assert b"conv_tap_group" in name_new and b"_narrow<" in name_new, name_new
        assert name_thr == name_new, (name_thr, name_new)          # (a group with a narrow member keeps its pointwise member under `throughput`)
        assert b"conv_tap_group" in name_old and b"narrow" not in name_old, name_old
        assert (b"conv_tap_group_pw_kernel" in name_new) == (b"conv_tap_group_pw_kernel" in name_old), (name_new, name_old)
        assert np.array_equal(new, sep), cfg
        assert np.array_equal(new, old), cfg
        assert np.array_equal(thr, sep), cfg
        g.check_against_reference(new)
    case.__name__ = "case_narrow_" + cfg
    case.__doc__ = "grouped launch %s: narrow form against separate launches, conv_group_narrow = 0 and ref_conv" % (CONFIGS[cfg],)
    return case


for _i, _cfg in enumerate(CONFIGS):
    globals()["case_narrow_" + _cfg] = _case(_cfg, 71 + _i)


def case_narrow_kernel_names(bk, golden):
    """The kernel-name contract: a group with a narrow member reports conv_tap_group[_pw]_kernel_narrow (still containing
    `conv_tap_group`, and `conv_tap_group_pw_kernel` when the pointwise member rides); under conv_group_narrow = 0, for a narrow
    member with Cin = 64, Cout = 128 or a residual, and for every group of the existing cases (all Cin >= 64) the name is today's;
    the default rule (conv_group_narrow = 1) leaves maps of a few tiles on today's launch."""
    rides = 0
    for cfg in ("bf16_28_16x32_pw", "f16_14_16x48_pw", "bf16_14_32x64_pw", "bf16_r25_8x24_pw", "bf16_28_32x96"):
        dt, shape, wide, narrow, pw = CONFIGS[cfg]
        g = _Group(bk, dt, shape, wide, narrow, pw, 5)
        yb = bk.dev(np.zeros(shape + (g.ctot,), NP_DT[dt]))
        items, keep = g.items(yb)
        buf = ctypes.create_string_buffer(256)
        names = {}
        for mode in (0, 1, 2):
            with _capi.options(bk.lib, conv_group_narrow=mode):
                assert bk.lib.step_conv_group_kernel_name(items, g.n, buf, 256) == 0
                names[mode] = buf.value
        t = b"step::bf16_t" if dt == BF16 else b"step::f16_t"
        assert names[0].startswith(b"void step::conv_tap_group") and b"_kernel<" + t + b", 0, " in names[0] and b"narrow" not in names[0], names
        assert names[1] == names[0], names                                    # (at most 21 boxes: below the default rule's tile count)
        pwk = b"conv_tap_group_pw_kernel" in names[0]
        rides += pwk
        assert names[2].startswith(b"void step::conv_tap_group" + (b"_pw" if pwk else b"") + b"_kernel_narrow<" + t + b", "), names
        assert (b"conv_tap_group_pw_kernel" in names[2]) == pwk
    assert rides >= 1, "no case carried its pointwise member"
    # not eligible: Cin = 64, Cout = 128 -> today's name under every option value
    for narrow in ((64, 40), (32, 128)):
        g = _Group(bk, BF16, MAP14, (64, 96), narrow, None, 6)
        yb = bk.dev(np.zeros(MAP14 + (g.ctot,), NP_DT[BF16]))
        items, keep = g.items(yb)
        buf = ctypes.create_string_buffer(256)
        seen = set()
        for mode in (0, 1, 2):
            with _capi.options(bk.lib, conv_group_narrow=mode):
                assert bk.lib.step_conv_group_kernel_name(items, 2, buf, 256) == 0
                seen.add(buf.value)
        assert len(seen) == 1 and b"conv_tap_group_kernel<step::bf16_t, 0, " in list(seen)[0], seen
    v = ctypes.c_int(-1)
    assert bk.lib.step_get_option(_capi.OPTION_IDS["conv_group_narrow"], ctypes.byref(v)) == 0 and v.value == 1
    assert bk.lib.step_set_option(_capi.OPTION_IDS["conv_group_narrow"], 3) != 0


def case_narrow_default_rule_c2_maps(bk, golden):
    """C2's own members (8 clips, 16 x 28 x 28 maps: Mixed_3b 96 -> 128 | 16 -> 32 with the pointwise 192 -> 32, Mixed_3c 128 -> 192 |
    32 -> 96 with 256 -> 64): the DEFAULT option value takes the narrow form (224 boxes of 4 x 4 x 28 per member), bit-identical to
    conv_group_narrow = 0 and to separate launches in both planner profiles."""
    for dt, wide, narrow, pw in ((BF16, (96, 128), (16, 32), (192, 32)), (BF16, (128, 192), (32, 96), (256, 64)), (F16, (128, 192), (32, 96), None)):
        g = _Group(bk, dt, (8, 16, 28, 28), wide, narrow, pw, 9)
        sep, _ = g.run(False)
        for prof in ({}, dict(throughput=1)):
            new, name = g.run(True, **prof)
            old, name_old = g.run(True, conv_group_narrow=0, **prof)
            assert b"_kernel_narrow<" in name and b"conv_tap_group" in name and b"narrow" not in name_old, (name, name_old)
            assert np.array_equal(new, sep) and np.array_equal(old, sep), (dt, narrow, prof)
        g.check_against_reference(new)
