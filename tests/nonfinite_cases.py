"""NaN / inf conformance of the forward kernels ("Non-finite contract"): non-finite values are planted in conv, stem, pool
and BN inputs and the outputs are compared CLASS BY CLASS (finite / +inf / -inf / NaN) with the plain operation in float64 on the
identically quantised inputs, rounded once to the storage type.  torch.relu, MaxPool3d and conv + BatchNorm3d + ReLU all propagate a
NaN; an fmaxf-style ReLU or max pool replaces it by a plausible number, and fp16 training with dynamic loss scaling then takes a
corrupt step (case_nf_fp16_step_is_skipped).  Driven on the host interpreter by tests/test_emul_nonfinite.py and on the real
library by tests/test_gpu_nonfinite.py -- the device build has its own staging code and its own max instructions (packed 16-bit
integer keys, v_pk_maximum3_f16), which the interpreter cannot see.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from step_amd import _capi
from tests import kernel_cases as KC
from tests.kernel_cases import BF16, F16, F32, NP_DT, cl, decode, encode, quantize, ref_conv, ref_stem, run_conv, run_stem, tol, uncl

DTS = (F32, BF16, F16)
NAN_POS = np.array([0x7fc00000], np.uint32).view(np.float32)[0]         # quiet NaNs by bit pattern; encode() keeps the sign in all
NAN_NEG = np.array([0xffc00000], np.uint32).view(np.float32)[0]         # three storage types (asserted in plant())
INF = np.float32(np.inf)


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def cls(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0))).astype(np.int8)


def to_storage(ref64, dt):
    """one rounding of the float64 reference to the storage type (overflow goes to inf, as in torch)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return quantize(np.asarray(ref64, np.float64).astype(np.float32), dt) if dt != F16 else np.asarray(ref64, np.float64).astype(np.float16).astype(np.float32)


def check(got, ref64, dt, what, atol=0.0, layers=1, bound=None):
    """class equality at EVERY element; |got - ref| <= tol(dt) * max finite |ref| (+ atol) where both are finite.  layers: storage
    roundings between input and output (two chained layers: the intermediate tensor's rounding may differ by one step from the
    double restatement's, which the second layer passes on -- 3 * tol, as case_conv_forward_pre_matches_two_launches).  bound: an
    absolute bound for the finite elements instead (where an existing case of the operator has its own)"""
    ref = to_storage(ref64, dt)
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    cg, cr = cls(got), cls(ref)
    bad = cg != cr
    assert not bad.any(), (what, "classes differ at %d of %d elements" % (int(bad.sum()), bad.size),
                           "reference finite/+inf/-inf/NaN %s" % np.bincount(cr.ravel(), minlength=4).tolist(),
                           "library %s" % np.bincount(cg.ravel(), minlength=4).tolist())
    fin = cr == 0
    if fin.any():
        if bound is None:
            bound = (1 if layers == 1 else 3) * tol(dt) * float(np.abs(ref[fin]).max()) + atol
        err = float(np.abs(got[fin].astype(np.float64) - ref[fin]).max())
        assert err <= bound, (what, err, bound)


def same(a, b, what):
    """two forms documented as bit-identical"""
    assert np.array_equal(a, b, equal_nan=True), (what, "differ at %d elements" % int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()))


def assert_planted_reference(ref64, dt, what, want=(0, 1, 2, 3)):
    """on the reference alone: the wanted classes all occur and at least a quarter of the outputs stay finite"""
    c = np.bincount(cls(to_storage(ref64, dt)).ravel(), minlength=4)
    assert all(c[k] > 0 for k in want), (what, c.tolist())
    assert c[0] * 4 >= c.sum(), (what, c.tolist())


# ---- the planting recipe ---------------------------------------------------------------------------------------------------------------
def plant(x, dt, caxis=1):
    """x: float32, channels on `caxis`; a copy with, at five pixels spread evenly over the remaining axes (flat order): a positive quiet
    NaN (channel 0), a negative quiet NaN (channel 1), a lone +inf (channel 2 % C), a lone -inf (channel 3 % C) and a +inf / -inf pair
    in channels 0 and C - 1 of ONE pixel (the accumulators themselves then produce NaN: inf - inf).  Tensors of fewer than 20 pixels
    use three pixels (the NaNs and the pair share the first one, in different channels), so that a quarter can stay finite.
    Returns the planted copy and the pixel indices."""
    x = np.moveaxis(np.array(x, np.float32, copy=True), caxis, -1)
    shp = x.shape
    C = shp[-1]
    assert C >= 3
    v = x.reshape(-1, C)
    P = v.shape[0]
    if P >= 20:
        pix = [(2 * k + 1) * P // 10 for k in range(5)]
    else:
        assert P >= 4
        pix = [0, 0, 1, 2, 0]
    v[pix[0], 0] = NAN_POS
    v[pix[1], 1] = NAN_NEG
    v[pix[2], 2 % C] = INF
    v[pix[3], 3 % C] = -INF
    pa, pb = (0, C - 1) if P >= 20 else (2, C - 1)
    v[pix[4], pa] = INF
    v[pix[4], pb] = -INF
    out = np.ascontiguousarray(np.moveaxis(v.reshape(shp), -1, caxis))
    e = encode(out, dt)
    bits = e.view(np.uint32 if dt == F32 else np.uint16)
    top = 31 if dt == F32 else 15
    nan = np.isnan(decode(e, dt))
    assert nan.sum() == 2 and sorted(((bits[nan] >> top) & 1).tolist()) == [0, 1], "the storage type holds one NaN of each sign"
    return out, pix


def conv_operands(case, seed=None):
    N, Cin, Cout, D, H, W, k = case
    rs = np.random.RandomState(Cin * 7 + Cout if seed is None else seed)
    x = rs.randn(N, Cin, D, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, *k) / np.sqrt(Cin * np.prod(k))).astype(np.float32)           # (as _conv_case: no finite sum comes near an overflow)
    scale = (1 + 0.1 * rs.randn(Cout)).astype(np.float32)
    shift = (0.2 * rs.randn(Cout)).astype(np.float32)
    return x, w, scale, shift


def conv_desc(case, dt, relu=1, res=False):
    """the descriptor run_conv(x_pad=(8, 8), y_pad=(16, 8)) builds -- for step_conv_kernel_name / step_conv_plan_info"""
    N, Cin, Cout, D, H, W, k = case
    return _capi.ConvDesc(dtype=dt, N=N, D=D, H=H, W=W, Cin=Cin, Cout=Cout, kd=k[0], kh=k[1], kw=k[2], x_cstride=Cin + 16, x_coff=8,
                          y_cstride=Cout + 24, y_coff=16, res_cstride=Cout if res else 0, res_coff=0, relu=relu, split=0, y2_cstride=0, y2_coff=0)


def kernel_name(bk, d):
    buf = ctypes.create_string_buffer(256)
    assert bk.lib.step_conv_kernel_name(ctypes.byref(d), buf, 256) == 0
    return buf.value.decode()


# ---- kernel cases (bk, golden) ---------------------------------------------------------------------------------------------------------
NF_CONV_SHAPES = [(1, 16, 32, 2, 8, 16, (3, 3, 3)), (2, 24, 48, 3, 9, 7, (3, 3, 3)), (1, 64, 40, 3, 9, 28, (3, 3, 3)), (2, 32, 40, 3, 7, 7, (1, 3, 3)),
                  (2, 72, 100, 2, 5, 9, (1, 1, 1)), (2, 264, 40, 1, 5, 9, (1, 1, 1))]
NF_CONV_ODD_COUT = (1, 64, 36, 2, 8, 16, (3, 3, 3))      # Cout % 8 != 0: the 16-bit tap kernel's element-store epilogue (no 16-byte stores)
NF_PWS_SHAPES = [(1, 64, 64, 2, 16, 33, (1, 1, 1)), (1, 192, 176, 1, 20, 53, (1, 1, 1)), (1, 144, 40, 2, 8, 67, (1, 1, 1)), (2, 32, 200, 1, 24, 23, (1, 1, 1))]
NF_SPLITK_SHAPES = [(5, 2056, 12, 1, 1, 1, (1, 1, 1)), (70, 2048, 60, 1, 1, 1, (1, 1, 1)), (1100, 1024, 12, 1, 1, 1, (1, 1, 1))]


def _nf_conv(bk, case, dts, seen, use_ws=False, relus=(1, 0), res=None):
    x, w, scale, shift = conv_operands(case)
    for dt in dts:
        xp, _ = plant(x, dt)
        for relu in relus:
            ref = ref_conv(xp, w, scale, shift, dt, relu=bool(relu), res=res, f64=True)
            assert_planted_reference(ref, dt, (case, dt, relu), want=(0, 1, 3) if relu else (0, 1, 2, 3))
            d = conv_desc(case, dt, relu, res is not None)
            info = (ctypes.c_int * 10)()
            assert bk.lib.step_conv_plan_info(ctypes.byref(d), info, 10) == 0
            vec = case[2] % 8 == 0
            seen.add((kernel_name(bk, d).split("<")[0].split("::")[-1] if not (use_ws and bk.lib.step_conv_workspace_bytes(ctypes.byref(d)) > 0) else "pw_splitk_kernel",
                      "f32" if dt == F32 else ("vec16" if vec else "elem16"), relu))
            got = run_conv(bk, xp, w, scale, shift, dt, relu=bool(relu), res=res, x_pad=(8, 8), y_pad=(16, 8), use_ws=use_ws, poison=np.nan)
            check(got, ref, dt, (case, dt, relu, use_ws))


def case_nf_conv_forms(bk, golden):
    """step_conv_forward with relu 1 and 0 through every form of the conv unit: the default planner, the four-wave and the eight-wave
    (classic / two-phase) tap kernel, the tiled kernel (conv_impl = 0), the streaming pointwise kernel (conv_impl = 5), the
    weight-stationary pointwise stream (conv_pws = 1) and split-K.  The operands sit in channel slices whose neighbours are NaN, so a
    kernel that reads a neighbour against a zero-padded weight (ragged K) shows; F32 and BF16 everywhere, F16 on the first shape of a form."""
    seen = set()

    def sweep(shapes, **kw):
        for i, case in enumerate(shapes):
            _nf_conv(bk, case, DTS if i == 0 else (F32, BF16), seen, **kw)

    sweep(NF_CONV_SHAPES + [NF_CONV_ODD_COUT])
    taps = [c for c in NF_CONV_SHAPES + [NF_CONV_ODD_COUT] if c[6] != (1, 1, 1)]
    with _capi.options(bk.lib, conv_waves=4):
        sweep(taps)
    with _capi.options(bk.lib, conv_waves=8):
        for ph in (0, 1, 2):
            with _capi.options(bk.lib, conv_phased=ph):
                sweep(taps)
    with _capi.options(bk.lib, conv_impl=0):
        sweep(NF_CONV_SHAPES)
    with _capi.options(bk.lib, conv_impl=5):
        sweep([c for c in NF_CONV_SHAPES if c[6] == (1, 1, 1)])
    with _capi.options(bk.lib, conv_pws=1):
        sweep(NF_PWS_SHAPES)
    sweep(NF_SPLITK_SHAPES, use_ws=True)
    planner = _capi.get_option(bk.lib, "conv_impl") == -1               # (a forced implementation bypasses the planner: only the names depend on it)
    if planner:
        # every epilogue of the conv unit was reached: the tap kernel's transposed 16-byte stores, its element stores (16-bit) and its
        # fp32 form, the streaming pointwise kernel's vector and element stores, the tiled kernel's, the weight-stationary stream's and
        # split-K's (conv_pw.hip)
        for want in (("conv_tap_kernel", "vec16"), ("conv_tap_kernel", "elem16"), ("conv_tap_kernel", "f32"), ("conv_pw_kernel", "vec16"),
                     ("conv_pw_kernel", "elem16"), ("conv_pw_kernel", "f32"), ("conv_igemm_kernel", "vec16"), ("conv_igemm_kernel", "f32"),
                     ("conv_pws_kernel", "vec16"), ("pw_splitk_kernel", "elem16"), ("pw_splitk_kernel", "f32")):
            assert any(k[:2] == want and k[2] == 1 for k in seen), (want, sorted(seen))
    # a non-finite RESIDUAL under relu = 1: the planted tensor is the residual, the conv's input is clean -- a pointwise layer (the heads'
    # Bottleneck conv3) and a 3x3x3 layer on the tap kernel (its 16-byte residual loads in 16-bit storage, element loads in fp32)
    for case in ((2, 32, 64, 1, 7, 7, (1, 1, 1)), (1, 64, 40, 3, 9, 28, (3, 3, 3))):
        x, w, scale, shift = conv_operands(case)
        rs = np.random.RandomState(3)
        for dt in DTS:
            res, _ = plant(rs.randn(case[0], case[2], *case[3:6]).astype(np.float32), dt)
            ref = ref_conv(x, w, scale, shift, dt, relu=True, res=res, f64=True)
            assert_planted_reference(ref, dt, ("residual", case, dt), want=(0, 1, 3))
            if planner and case[6] == (3, 3, 3):
                assert "conv_tap_kernel" in kernel_name(bk, conv_desc(case, dt, 1, True))
            got = run_conv(bk, x, w, scale, shift, dt, relu=True, res=res, x_pad=(8, 8), y_pad=(16, 8), poison=np.nan)
            check(got, ref, dt, ("residual", case, dt))


def case_nf_stem(bk, golden):
    """step_stem_forward on x [1,4,3,16,16], Cout 64, in all three storage types against ref_stem in double; step_stem_pool_forward at the
    smallest shape of case_stem_pool_fused against the stem followed by the pool (bit-identical, NaN == NaN) and against the double
    restatement by class."""
    rs = np.random.RandomState(17)
    Cout = 64
    w = (rs.randn(Cout, 3, 7, 7, 7) / np.sqrt(1029)).astype(np.float32)
    scale = (1 + 0.1 * rs.randn(Cout)).astype(np.float32)
    shift = (0.2 * rs.randn(Cout)).astype(np.float32)
    x0 = rs.randn(1, 4, 3, 16, 16).astype(np.float32)
    for dt in DTS:
        x, _ = plant(x0, dt, caxis=2)
        ref = ref_stem(x, w, scale, shift, dt, f64=True)
        assert_planted_reference(ref, dt, ("stem", dt), want=(0, 1, 3))
        check(run_stem(bk, x, w, scale, shift, dt), ref, dt, ("stem", dt))
    N, T, H, W = 1, 2, 20, 24
    ycs, yoff = 80, 8
    x0 = rs.uniform(-1, 1, (N, T, 3, H, W)).astype(np.float32)
    for dt in (BF16, F16):
        x, _ = plant(x0, dt, caxis=2)
        To, Ho, Wo = (T - 2) // 2 + 1, (H - 2) // 2 + 1, (W - 2) // 2 + 1
        Hp, Wp = bk.lib.step_pool_out_size(Ho, 3, 2), bk.lib.step_pool_out_size(Wo, 3, 2)
        wp = bk.dev(np.zeros(bk.lib.step_stem_packed_elems(Cout), NP_DT[dt]))
        wd = bk.dev(np.ascontiguousarray(w, np.float32))
        assert bk.lib.step_stem_pack_weight(wd.ptr, Cout, dt, wp.ptr, bk.stream) == 0
        xe, sc, sh = bk.dev(encode(x, dt)), bk.dev(scale), bk.dev(shift)
        y = bk.dev(np.zeros((N, To, Ho, Wo, Cout), NP_DT[dt]))
        assert bk.lib.step_stem_forward(dt, xe.ptr, N, T, H, W, wp.ptr, sc.ptr, sh.ptr, 1, Cout, y.ptr, Cout, 0, bk.stream) == 0
        sep = bk.dev(np.zeros((N, To, Hp, Wp, Cout), NP_DT[dt]))
        assert bk.lib.step_maxpool3d_tf(dt, y.ptr, N, To, Ho, Wo, Cout, Cout, 0, 1, 3, 3, 1, 2, 2, sep.ptr, Cout, 0, bk.stream) == 0
        wsb = bk.lib.step_stem_pool_workspace_bytes(dt, N, T, H, W, Cout)
        assert wsb > 0
        ws = bk.dev(np.full(wsb // 2, 0x7f7f, np.uint16))
        out = bk.dev(np.zeros((N, To, Hp, Wp, ycs), NP_DT[dt]))
        assert bk.lib.step_stem_pool_forward(dt, xe.ptr, N, T, H, W, wp.ptr, sc.ptr, sh.ptr, Cout, out.ptr, ycs, yoff, ws.ptr, wsb, bk.stream) == 0
        fused = decode(out.get(), dt)
        assert not fused[..., :yoff].any() and not fused[..., yoff + Cout:].any()
        sepf = decode(sep.get(), dt)
        ref = pool_ref(torch.from_numpy(to_storage(ref_stem(x, w, scale, shift, dt, f64=True), dt)).double(), (1, 3, 3), (1, 2, 2))
        assert_planted_reference(ref, dt, ("stem_pool", dt), want=(0, 1, 3))
        check(uncl(sepf), ref, dt, ("stem then pool", dt))
        same(fused[..., yoff:yoff + Cout], sepf, ("stem_pool vs stem + pool", dt))


def pool_ref(x, k, s):
    """MaxPool3dTFPadding in double: F.max_pool3d(ceil_mode) on the explicitly zero-padded tensor (x NCDHW, a torch tensor)"""
    pads = []
    for kk, ss in zip(reversed(k), reversed(s)):
        t = max(kk - ss, 0)
        pads += [t // 2, t - t // 2]
    return F.max_pool3d(F.pad(x.double(), pads), k, s, ceil_mode=True).numpy()


NF_POOLS = (((3, 3, 3), (1, 1, 1)), ((1, 3, 3), (1, 2, 2)), ((2, 2, 2), (2, 2, 2)))


def case_nf_maxpool(bk, golden):
    """step_maxpool3d_tf on [1,4,9,9,16] and a 40-channel variant (ragged channel chunk: 40 = 32 + 8), three windows, three storage types,
    the separable kernels (pool_direct = 0) and the direct one: a NaN of EITHER sign wins its windows (the bf16 pool orders integer keys,
    the fp16 pool is a packed instruction, the fp32 pool and the interpreter compare floats -- one rule for all), +inf wins, -inf loses to
    everything -- also to the zeros of the TF padding -- and a window that holds nothing but -inf gives -inf."""
    rs = np.random.RandomState(23)
    for C in (16, 40):
        x0 = rs.randn(1, C, 4, 9, 9).astype(np.float32)
        for dt in DTS:
            x, _ = plant(x0, dt)
            x[0, 5, 0:2, 0:2, 0:2] = -INF               # (2,2,2)/2: a whole window of -inf (no padding there); (3,3,3)/1 at the corner: -inf and pad zeros only
            x[0, 6, 3, 8, 8] = NAN_NEG                  # a NaN beside the padding
            x[0, 7, 0, 0, 8] = NAN_POS
            xq = torch.from_numpy(quantize(x, dt))
            for k, s in NF_POOLS:
                ref = pool_ref(xq, k, s)
                assert_planted_reference(ref, dt, ("pool", C, dt, k), want=(0, 1, 2, 3) if k == (2, 2, 2) else (0, 1, 3))
                Do, Ho, Wo = (bk.lib.step_pool_out_size(a, b, c) for a, b, c in zip((4, 9, 9), k, s))
                assert ref.shape == (1, C, Do, Ho, Wo)
                outs = []
                for direct in (0, 1):
                    with _capi.options(bk.lib, pool_direct=direct):
                        xb = np.full((1, 4, 9, 9, C + 16), np.nan, np.float32)      # input as a channel slice with NaN neighbours
                        xb[..., 8:8 + C] = cl(x)
                        xd = bk.dev(encode(xb, dt))
                        y = bk.dev(np.zeros((1, Do, Ho, Wo, C + 8), NP_DT[dt]))
                        assert bk.lib.step_maxpool3d_tf(dt, xd.ptr, 1, 4, 9, 9, C, C + 16, 8, k[0], k[1], k[2], s[0], s[1], s[2], y.ptr, C + 8, 8, bk.stream) == 0
                        yy = decode(y.get(), dt)
                        assert not yy[..., :8].any()
                        got = uncl(yy[..., 8:])
                        check(got, ref, dt, ("pool", C, dt, k, s, direct))
                        fin = np.isfinite(ref)
                        assert np.array_equal(got[fin], ref[fin].astype(np.float32)), ("a max pool rounds nothing", C, dt, k, direct)
                        outs.append(got)
                same(outs[0], outs[1], ("pool_direct 0 vs 1", C, dt, k))


def case_nf_bn_train(bk, golden):
    """step_bn_train_forward (relu 1 and 0), M = 70, C = 8, against torch batch_norm(training=True) + relu in double: one NaN in channel 0
    makes that channel's statistics NaN, so the WHOLE channel is NaN (an fmaxf ReLU made it all zeros) and the others are untouched;
    save_mean / save_invstd / the running statistics by class.  step_avgpool_hw on [1,2,5,5,8], window 3x3, against numpy."""
    rs = np.random.RandomState(29)
    M, C = 70, 8
    z0 = (rs.randn(M, C) * rs.uniform(0.5, 2.0, C) + rs.uniform(-3, 3, C)).astype(np.float32)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(np.float32), rs.uniform(-1, 1, C).astype(np.float32)
    rm0, rv0 = rs.randn(C).astype(np.float32), rs.uniform(0.5, 2, C).astype(np.float32)
    for dt in DTS:
        for relu in (1, 0):
            z = z0.copy()
            z[33, 0] = NAN_NEG
            zq = quantize(z, dt)
            rm, rv = torch.from_numpy(rm0.astype(np.float64)), torch.from_numpy(rv0.astype(np.float64))
            yr = F.batch_norm(torch.from_numpy(zq).double().t().reshape(1, C, M), rm, rv, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(),
                              True, 0.1, 1e-5).reshape(C, M).t()
            yr = (F.relu(yr) if relu else yr).numpy()
            assert np.isnan(yr[:, 0]).all() and np.isfinite(yr[:, 1:]).all()
            Z, Y = bk.dev(encode(zq, dt)), bk.dev(np.zeros((M, C), NP_DT[dt]))
            G, Bt = bk.dev(gamma), bk.dev(beta)
            RM, RV = bk.dev(rm0.copy()), bk.dev(rv0.copy())
            SM, SI = bk.dev(np.zeros(C, np.float32)), bk.dev(np.zeros(C, np.float32))
            wsb = bk.lib.step_bn_train_workspace_bytes(M, C)
            WS = bk.dev(np.full(wsb // 4 + 4, np.nan, np.float32))
            assert bk.lib.step_bn_train_forward(dt, Z.ptr, C, M, C, G.ptr, Bt.ptr, 1e-5, 0.1, RM.ptr, RV.ptr, SM.ptr, SI.ptr, relu, Y.ptr, C, WS.ptr, wsb,
                                                bk.stream) == 0
            check(decode(Y.get(), dt), yr, dt, ("bn_train", dt, relu), atol=2e-5)
            mean, var = zq.astype(np.float64).mean(0), zq.astype(np.float64).var(0)
            check(SM.get(), mean, F32, ("save_mean", dt), atol=1e-6)
            check(SI.get(), 1 / np.sqrt(var + 1e-5), F32, ("save_invstd", dt))
            check(RM.get(), rm.numpy(), F32, ("running_mean", dt))
            check(RV.get(), rv.numpy(), F32, ("running_var", dt))
    x = rs.randn(1, 8, 2, 5, 5).astype(np.float32)
    x[0, 0, 0, 2, 2], x[0, 1, 1, 0, 0], x[0, 2, 0, 4, 4], x[0, 3, 1, 0, 4], x[0, 3, 1, 2, 4] = NAN_POS, INF, -INF, INF, -INF
    for dt in DTS:
        xq = quantize(x, dt).astype(np.float64)
        with np.errstate(invalid="ignore"):
            ref = np.stack([np.stack([xq[:, :, :, i:i + 3, j:j + 3].sum((3, 4)) / 9.0 for j in range(3)], -1) for i in range(3)], -2)
        assert_planted_reference(ref, dt, ("avgpool", dt))
        xd, y = bk.dev(encode(cl(x), dt)), bk.dev(np.zeros((1, 2, 3, 3, 8), NP_DT[dt]))
        assert bk.lib.step_avgpool_hw(dt, xd.ptr, 1, 2, 5, 5, 8, 3, 3, y.ptr, bk.stream) == 0
        check(uncl(decode(y.get(), dt)), ref, dt, ("avgpool", dt), atol=1e-6)


def _item(items, k, d, x, wp, sc, sh, y):
    it = items[k]
    it.desc = ctypes.pointer(d)
    it.x, it.w_packed, it.scale, it.shift, it.res, it.y = (ctypes.cast(p, ctypes.c_void_p).value for p in (x.ptr, wp.ptr, sc.ptr, sh.ptr, None, y.ptr))
    it.res = None


def _desc(dt, N, D, H, W, Cin, Cout, k, xcs, xco, ycs, yco, relu=1, split=0, y2cs=0, y2co=0, res=0):
    return _capi.ConvDesc(dtype=dt, N=N, D=D, H=H, W=W, Cin=Cin, Cout=Cout, kd=k, kh=k, kw=k, x_cstride=xcs, x_coff=xco, y_cstride=ycs, y_coff=yco,
                          res_cstride=res, res_coff=0, relu=relu, split=split, y2_cstride=y2cs, y2_coff=y2co)


def _affine(rs, C):
    return (1 + 0.1 * rs.randn(C)).astype(np.float32), (0.2 * rs.randn(C)).astype(np.float32)


def case_nf_conv_fused_forms(bk, golden):
    """Every fused call equals its separate calls on planted inputs, NaN == NaN (np.array_equal(equal_nan=True)), and the separate calls
    equal the double restatement by class: step_conv_forward_pre, step_conv_forward_pre_pool (the persistent tile loop and conv_persist
    = 0), step_pool_conv_forward, step_conv_forward_group and step_conv_forward_cat, each on the first shape and option set of its
    *_matches_* case.  The pooled epilogues order 16-bit patterns as integers: a NaN of either sign comes out of them as NaN."""
    rs = np.random.RandomState(41)
    dt = BF16
    # ---- step_conv_forward_pre, step_conv_forward_pre_pool
    for (N, D, H, W), Cout, opts in (((1, 4, 24, 24), 192, dict(conv_slots=4, conv_nb=3, conv_waves=8)),
                                     ((1, 8, 24, 24), 192, dict(conv_slots=8, conv_nb=3, conv_waves=8, conv_gen=0, conv_persist=0))):
        x, _ = plant(rs.randn(N, 64, D, H, W).astype(np.float32), dt)
        wa = (rs.randn(64, 64, 1, 1, 1) / 8).astype(np.float32)
        wb = (rs.randn(Cout, 64, 3, 3, 3) / np.sqrt(64 * 27)).astype(np.float32)
        (sa, ha), (sb, hb) = _affine(rs, 64), _affine(rs, Cout)
        mid64 = ref_conv(x, wa, sa, ha, dt, f64=True)
        ref = ref_conv(to_storage(mid64, dt), wb, sb, hb, dt, f64=True)
        # (the pointwise layer turns a planted inf into +inf in about half of its 64 channels; the 3x3x3 layer then sums them with
        # weights of both signs -- inf - inf: the chain's output holds NaN and finite values, the intermediate tensor all three classes)
        assert_planted_reference(mid64, dt, ("pre: pointwise layer", N, D), want=(0, 1, 3))
        assert_planted_reference(ref, dt, ("pre", N, D), want=(0, 3))
        xe = bk.dev(encode(cl(x), dt))
        wpa, wpb = KC.pack_weight(bk, wa, dt), KC.pack_weight(bk, wb, dt)
        dsa, dha, dsb, dhb = bk.dev(sa), bk.dev(ha), bk.dev(sb), bk.dev(hb)
        Hp, Wp = bk.lib.step_pool_out_size(H, 3, 2), bk.lib.step_pool_out_size(W, 3, 2)
        da, db = _desc(dt, N, D, H, W, 64, 64, 1, 64, 0, 64, 0), _desc(dt, N, D, H, W, 64, Cout, 3, 64, 0, Cout, 0)
        with _capi.options(bk.lib, **opts):
            mid = bk.dev(np.zeros((N, D, H, W, 64), NP_DT[dt]))
            y2 = bk.dev(np.zeros((N, D, H, W, Cout), NP_DT[dt]))
            assert bk.lib.step_conv_forward(ctypes.byref(da), xe.ptr, wpa.ptr, dsa.ptr, dha.ptr, None, mid.ptr, None, bk.stream) == 0
            assert bk.lib.step_conv_forward(ctypes.byref(db), mid.ptr, wpb.ptr, dsb.ptr, dhb.ptr, None, y2.ptr, None, bk.stream) == 0
            check(uncl(decode(mid.get(), dt)), mid64, dt, ("pre: pointwise layer", N, D))
            sep = decode(y2.get(), dt)
            check(uncl(sep), ref, dt, ("pre: separate calls", N, D), layers=2)
            y1 = bk.dev(np.full((N, D, H, W, Cout), 7, NP_DT[dt]))
            assert bk.lib.step_conv_forward_pre(ctypes.byref(db), xe.ptr, wpb.ptr, dsb.ptr, dhb.ptr, wpa.ptr, dsa.ptr, dha.ptr, 64, y1.ptr, bk.stream) == 0
            same(decode(y1.get(), dt), sep, ("conv_forward_pre vs two launches", N, D))
            want = bk.dev(np.zeros((N, D, Hp, Wp, Cout), NP_DT[dt]))
            assert bk.lib.step_maxpool3d_tf(dt, y2.ptr, N, D, H, W, Cout, Cout, 0, 1, 3, 3, 1, 2, 2, want.ptr, Cout, 0, bk.stream) == 0
            pooled = decode(want.get(), dt)
            pref = pool_ref(torch.from_numpy(uncl(sep)), (1, 3, 3), (1, 2, 2))          # the pool of the separate calls' own output: exact
            assert (cls(pooled) == 3).any()
            assert np.array_equal(uncl(pooled), pref.astype(np.float32), equal_nan=True), ("pool of the separate calls", N, D)
            nb = bk.lib.step_conv_pre_pool_workspace_bytes(ctypes.byref(db))
            assert nb > 0
            info = (ctypes.c_int * 13)()
            assert bk.lib.step_conv_pre_pool_plan_info(ctypes.byref(db), info, 13) == 0
            assert info[0] == 1 and info[1] == 3 and info[4] == 1, list(info)                  # conv_tap, the 4 x 8 x 8 tile, two-phase
            assert (info[12] > 0) == ("conv_persist" not in opts), list(info)                  # the persistent tile loop | one workgroup per tile
            ws = bk.dev(np.full(nb // 2, 0x7f7f, np.uint16))
            got = bk.dev(np.full((N, D, Hp, Wp, Cout), 3, NP_DT[dt]))
            assert bk.lib.step_conv_forward_pre_pool(ctypes.byref(db), xe.ptr, wpb.ptr, dsb.ptr, dhb.ptr, wpa.ptr, dsa.ptr, dha.ptr, 64, got.ptr,
                                                     ws.ptr, nb, bk.stream) == 0
            same(decode(got.get(), dt), pooled, ("conv_forward_pre_pool vs separate calls", N, D, opts))
    # ---- step_pool_conv_forward
    (N, D, H, W), Cin, Cout, split = (8, 3, 14, 14), 136, 104, 40
    x, _ = plant(rs.randn(N, Cin, D, H, W).astype(np.float32), dt)
    w = (rs.randn(Cout, Cin, 1, 1, 1) / np.sqrt(Cin)).astype(np.float32)
    sc, sh = _affine(rs, Cout)
    xe, wp, dsc, dsh = bk.dev(encode(cl(x), dt)), KC.pack_weight(bk, w, dt), bk.dev(sc), bk.dev(sh)
    d = _desc(dt, N, D, H, W, Cin, Cout, 1, Cin, 0, split + 8, 8, split=split, y2cs=Cout - split)
    outs = []
    for fused in (True, False):
        py = bk.dev(np.full((N, D, H, W, Cin), 3, NP_DT[dt]))
        y, y2 = bk.dev(np.zeros((N, D, H, W, split + 8), NP_DT[dt])), bk.dev(np.zeros((N, D, H, W, Cout - split), NP_DT[dt]))
        if fused:
            assert bk.lib.step_pool_conv_forward(dt, xe.ptr, N, D, H, W, Cin, Cin, 0, py.ptr, Cin, 0, ctypes.byref(d), xe.ptr, wp.ptr, dsc.ptr, dsh.ptr,
                                                 y.ptr, y2.ptr, bk.stream) == 0
        else:
            assert bk.lib.step_maxpool3d_tf(dt, xe.ptr, N, D, H, W, Cin, Cin, 0, 3, 3, 3, 1, 1, 1, py.ptr, Cin, 0, bk.stream) == 0
            assert bk.lib.step_conv_forward(ctypes.byref(d), xe.ptr, wp.ptr, dsc.ptr, dsh.ptr, None, y.ptr, y2.ptr, bk.stream) == 0
        outs.append([decode(a.get(), dt) for a in (py, y, y2)])
    pref = pool_ref(torch.from_numpy(quantize(x, dt)), (3, 3, 3), (1, 1, 1))
    assert_planted_reference(pref, dt, "pool_conv: pool", want=(0, 1, 3))
    check(uncl(outs[1][0]), pref, dt, "pool_conv: separate pool")
    cref = ref_conv(x, w, sc, sh, dt, f64=True)
    assert_planted_reference(cref, dt, "pool_conv: conv", want=(0, 1, 3))
    check(np.concatenate([uncl(outs[1][1][..., 8:]), uncl(outs[1][2])], 1), cref, dt, "pool_conv: separate conv")
    for a, b, what in zip(outs[0], outs[1], ("pooled", "y", "y2")):
        same(a, b, ("pool_conv_forward vs two launches", what))
    # ---- step_conv_forward_group (both members on the partner's instantiation: Cin = 64)
    (N, D, H, W), (ci0, co0, ci1, co1) = (1, 8, 14, 14), (64, 200, 64, 40)
    t, _ = plant(rs.randn(N, ci0 + ci1, D, H, W).astype(np.float32), dt)
    t[0, ci0 + 1, 5, 7, 7] = NAN_NEG                          # (the second member's slice gets a NaN of its own)
    wsg = [(rs.randn(co, ci, 3, 3, 3) / np.sqrt(ci * 27)).astype(np.float32) for ci, co in ((ci0, co0), (ci1, co1))]
    aff = [_affine(rs, co) for co in (co0, co1)]
    te = bk.dev(encode(cl(t), dt))
    ctot = 8 + co0 + co1 + 8
    outs, buf = [], ctypes.create_string_buffer(256)
    for grouped in (True, False):
        yb = bk.dev(np.zeros((N, D, H, W, ctot), NP_DT[dt]))
        keep, items = [], (_capi.ConvItem * 2)()
        for k_, (ci, co, xoff, yoff) in enumerate(((ci0, co0, 0, 8), (ci1, co1, ci0, 8 + co0))):
            dg = _desc(dt, N, D, H, W, ci, co, 3, ci0 + ci1, xoff, ctot, yoff)
            wpk, scg, shg = KC.pack_weight(bk, wsg[k_], dt), bk.dev(aff[k_][0]), bk.dev(aff[k_][1])
            keep += [dg, wpk, scg, shg]
            _item(items, k_, dg, te, wpk, scg, shg, yb)
        if grouped:
            assert bk.lib.step_conv_group_kernel_name(items, 2, buf, 256) == 0
            if _capi.get_option(bk.lib, "conv_impl") == -1:
                assert b"conv_tap_group_kernel" in buf.value, buf.value
            assert bk.lib.step_conv_forward_group(items, 2, bk.stream) == 0
        else:
            for k_ in range(2):
                it = items[k_]
                assert bk.lib.step_conv_forward(it.desc, it.x, it.w_packed, it.scale, it.shift, None, it.y, None, bk.stream) == 0
        outs.append(decode(yb.get(), dt))
    same(outs[0], outs[1], "conv_forward_group vs separate launches")
    assert not outs[1][..., :8].any() and not outs[1][..., 8 + co0 + co1:].any()
    for k_, (lo, hi, xlo, xhi) in enumerate(((8, 8 + co0, 0, ci0), (8 + co0, 8 + co0 + co1, ci0, ci0 + ci1))):
        ref = ref_conv(t[:, xlo:xhi], wsg[k_], aff[k_][0], aff[k_][1], dt, f64=True)
        assert_planted_reference(ref, dt, ("group member", k_), want=(0, 1, 3))
        check(uncl(outs[1][..., lo:hi]), ref, dt, ("group member, separate launch", k_))
    # ---- step_conv_forward_group with a member on the pixel-split form (conv_tap_narrow.h: Cin <= 32, Cout <= 96; conv_group_narrow = 2 takes
    # it on maps this small): the shared input buffer has NaN channels on both sides, relu 1 and 0, the 16-byte epilogue (Cout 64) and
    # the element one (Cout 44)
    N, D, H, W = 5, 8, 14, 14
    for gdt, (ci1, co1) in ((BF16, (24, 64)), (F16, (32, 44))):
        ci0, co0 = 64, 64
        t, _ = plant(rs.randn(N, ci0 + ci1, D, H, W).astype(np.float32), gdt)
        t[2, ci0, 3, 5, 5], t[2, ci0 + 1, 6, 9, 2], t[3, ci0 + 2, 1, 12, 12], t[3, ci0 + 3, 4, 2, 9] = NAN_POS, NAN_NEG, INF, -INF   # (the narrow member's own plants;
        t[4, ci0 + 4, 5, 7, 7] = -INF                                                                                    # plant() put +inf / -inf into channels 0 and C - 1)
        tb = np.full((N, D, H, W, 8 + ci0 + ci1 + 8), np.nan, np.float32)
        tb[..., 8:8 + ci0 + ci1] = cl(t)
        te = bk.dev(encode(tb, gdt))
        wsg = [(rs.randn(co, ci, 3, 3, 3) / np.sqrt(ci * 27)).astype(np.float32) for ci, co in ((ci0, co0), (ci1, co1))]
        aff = [_affine(rs, co) for co in (co0, co1)]
        ctot = 8 + co0 + co1 + 8 + (4 if co1 % 8 else 0)
        for relu in (1, 0):
            outs = []
            for grouped in (True, False):
                yb = bk.dev(np.zeros((N, D, H, W, ctot), NP_DT[gdt]))
                keep, items = [], (_capi.ConvItem * 2)()
                for k_, (ci, co, xoff, yoff) in enumerate(((ci0, co0, 8, 8), (ci1, co1, 8 + ci0, 8 + co0))):
                    dg = _desc(gdt, N, D, H, W, ci, co, 3, tb.shape[-1], xoff, ctot, yoff, relu=relu)
                    wpk, scg, shg = KC.pack_weight(bk, wsg[k_], gdt), bk.dev(aff[k_][0]), bk.dev(aff[k_][1])
                    keep += [dg, wpk, scg, shg]
                    _item(items, k_, dg, te, wpk, scg, shg, yb)
                with _capi.options(bk.lib, conv_group_narrow=2):
                    if grouped:
                        assert bk.lib.step_conv_group_kernel_name(items, 2, buf, 256) == 0
                        if _capi.get_option(bk.lib, "conv_impl") == -1:
                            assert b"conv_tap_group" in buf.value and b"_narrow<" in buf.value, buf.value
                        assert bk.lib.step_conv_forward_group(items, 2, bk.stream) == 0
                    else:
                        for k_ in range(2):
                            it = items[k_]
                            assert bk.lib.step_conv_forward(it.desc, it.x, it.w_packed, it.scale, it.shift, None, it.y, None, bk.stream) == 0
                outs.append(decode(yb.get(), gdt))
            same(outs[0], outs[1], ("conv_forward_group with a narrow member vs separate launches", gdt, relu))
            assert not outs[0][..., :8].any() and not outs[0][..., 8 + co0 + co1:].any()
            for k_, (lo, hi, xlo, xhi) in enumerate(((8, 8 + co0, 0, ci0), (8 + co0, 8 + co0 + co1, ci0, ci0 + ci1))):
                ref = ref_conv(t[:, xlo:xhi], wsg[k_], aff[k_][0], aff[k_][1], gdt, relu=bool(relu), f64=True)
                assert_planted_reference(ref, gdt, ("narrow group member", k_, relu), want=(0, 1, 3) if relu else (0, 1, 2, 3))
                check(uncl(outs[0][..., lo:hi]), ref, gdt, ("narrow group member, grouped launch", gdt, k_, relu))
    # ---- step_conv_forward_cat (both sources are channel slices with NaN neighbours; a non-finite residual)
    N, Ca, Cb, Cout, D, H, W, ap, bp = 1, 96, 72, 136, 1, 64, 65, (32, 8), (8, 16)
    xa, _ = plant(rs.randn(N, Ca, D, H, W).astype(np.float32), dt)
    xb = rs.randn(N, Cb, D, H, W).astype(np.float32)
    xb[0, 5, 0, 40, 40], xb[0, Cb - 1, 0, 50, 3] = NAN_NEG, INF
    w = (rs.randn(Cout, Ca + Cb, 1, 1, 1) / np.sqrt(Ca + Cb)).astype(np.float32)
    sc, sh = _affine(rs, Cout)
    r = rs.randn(N, Cout, D, H, W).astype(np.float32)
    r[0, 7, 0, 9, 9], r[0, 8, 0, 9, 9] = NAN_POS, -INF
    xc = np.concatenate([xa, xb], 1)
    ref = ref_conv(xc, w, sc, sh, dt, relu=True, res=r, f64=True)
    assert_planted_reference(ref, dt, "cat", want=(0, 1, 3))
    ab = np.full((N, D, H, W, ap[0] + Ca + ap[1]), np.nan, np.float32)
    ab[..., ap[0]:ap[0] + Ca] = cl(xa)
    bb = np.full((N, D, H, W, bp[0] + Cb + bp[1]), np.nan, np.float32)
    bb[..., bp[0]:bp[0] + Cb] = cl(xb)
    ae, be, ce, re_ = bk.dev(encode(ab, dt)), bk.dev(encode(bb, dt)), bk.dev(encode(cl(xc), dt)), bk.dev(encode(cl(r), dt))
    wp, dsc, dsh = KC.pack_weight(bk, w, dt), bk.dev(sc), bk.dev(sh)
    y1, y2 = bk.dev(np.zeros((N, D, H, W, Cout), NP_DT[dt])), bk.dev(np.zeros((N, D, H, W, Cout), NP_DT[dt]))
    dcat = _desc(dt, N, D, H, W, Ca + Cb, Cout, 1, ab.shape[-1], ap[0], Cout, 0, res=Cout)
    assert bk.lib.step_conv_forward_cat(ctypes.byref(dcat), ae.ptr, Ca, be.ptr, bb.shape[-1], bp[0], wp.ptr, dsc.ptr, dsh.ptr, re_.ptr, y1.ptr, None, bk.stream) == 0
    dc = _desc(dt, N, D, H, W, Ca + Cb, Cout, 1, Ca + Cb, 0, Cout, 0, res=Cout)
    assert bk.lib.step_conv_forward(ctypes.byref(dc), ce.ptr, wp.ptr, dsc.ptr, dsh.ptr, re_.ptr, y2.ptr, None, bk.stream) == 0
    check(uncl(decode(y2.get(), dt)), ref, dt, "cat: conv on the materialised concat")
    same(decode(y1.get(), dt), decode(y2.get(), dt), "conv_forward_cat vs the materialised concat")


NF_WGRAD_SHAPES = [(2, 24, 40, 3, 5, 19, (3, 3, 3)), (1, 72, 100, 2, 6, 7, (1, 3, 3)), (1, 40, 70, 1, 9, 130, (1, 1, 1)),
                   (1, 64, 72, 3, 20, 14, (3, 3, 3)), (1, 392, 72, 2, 9, 40, (1, 1, 1)), (1, 72, 40, 2, 36, 40, (1, 1, 1))]


def wgrad_ref(xq, gq, k, skip=None):
    """dw[co, ci, taps] in float64: the sum over the pixels INSIDE the image of dy[co, p] * x[ci, p + tap] (the zero padding is no operand:
    a tap that leaves the image from pixel p has no term for p).  skip = (n, co, d, h, w): that element of dy is left out."""
    g = np.array(gq, np.float64)
    if skip is not None:
        g[skip] = 0.0
    w = torch.zeros(g.shape[1], xq.shape[1], *k, dtype=torch.float64, requires_grad=True)
    F.conv3d(torch.from_numpy(np.asarray(xq, np.float64)), w, padding=tuple(kk // 2 for kk in k)).backward(torch.from_numpy(g))
    return w.grad.numpy()


def case_nf_wgrad_sliced_operands(bk, golden):
    """The five weight-gradient entry points with BOTH operands read in place as channel slices whose neighbours are NaN (x: 8 NaN channels
    on each side; dy: y_cstride = Cout + 24, y_coff = 16 -- how ops._wgrad_setup reads an Inception block's gradients) and NaN-filled
    scratch: with finite operands dw holds no NaN and is within 2e-5 of torch autograd; with ONE +inf inside dy's slice exactly the rows
    dw[co, :, taps] of that channel, at the taps that reach the pixel from inside the image, are +-inf (the sign of the x they meet)."""
    rs = np.random.RandomState(43)
    try:
        for minpix, ldsopt in ((64, 0), (0, 1), (0, 2)):
            _capi.set_option(bk.lib, "wgrad_minpix", minpix)
            _capi.set_option(bk.lib, "wgrad16_lds", ldsopt)
            for (N, Cin, Cout, D, H, W, k) in NF_WGRAD_SHAPES:
                x = rs.randn(N, Cin, D, H, W).astype(np.float32)
                gy = rs.randn(N, Cout, D, H, W).astype(np.float32)
                # the +inf: an interior pixel wherever the map has one.  Every tap that stays inside the image from there meets a real x; a
                # tap that leaves the image has NO term in the einsum over image pixels, while kernels that stage the halo as zeros (and a
                # plain einsum over the padded tensor) compute inf x 0 = NaN there -- both are "non-finite rows of that channel", so the
                # planted pixel is chosen where the two readings agree: every tap reaches it on all six maps (asserted below)
                hot = (N - 1, Cout // 2, D // 2, H // 2, W // 2)
                for dt, w16 in ((F32, False), (BF16, True), (F16, True)):
                    gdt = dt if w16 else F32
                    xq, gq = quantize(x, dt), quantize(gy, gdt)
                    assert (xq != 0).all()
                    d = _capi.ConvDesc(dtype=dt, N=N, D=D, H=H, W=W, Cin=Cin, Cout=Cout, kd=k[0], kh=k[1], kw=k[2], x_cstride=Cin + 16, x_coff=8,
                                       y_cstride=Cout + 24, y_coff=16, res_cstride=0, res_coff=0, relu=0, split=0, y2_cstride=0, y2_coff=0)
                    xb = np.full((N, D, H, W, Cin + 16), np.nan, np.float32)
                    xb[..., 8:8 + Cin] = cl(xq)
                    xd = bk.dev(encode(xb, dt))
                    nbw = (bk.lib.step_conv_wgrad16_workspace_bytes if w16 else bk.lib.step_conv_wgrad_workspace_bytes)(ctypes.byref(d))
                    plain, with_ws = (bk.lib.step_conv_wgrad16, bk.lib.step_conv_wgrad16_ws) if w16 else (bk.lib.step_conv_wgrad, bk.lib.step_conv_wgrad_ws)
                    # "border": the same +inf on the map's left border, where the taps kw = 0 leave the image.  The einsum has no term there;
                    # the kernels stage the halo as zeros and multiply, inf x 0 = NaN: the documented behaviour, pinned
                    # here -- those taps of that channel are NaN, the taps that reach the pixel +-inf, nothing else in dw changes
                    for planted in (False, "interior", "border") if k[2] == 3 else (False, "interior"):
                        g = gq.copy()
                        if planted:
                            h_ = hot if planted == "interior" else hot[:4] + (0,)
                            g[h_] = INF
                            ref = wgrad_ref(xq, gq, k, skip=h_)
                            n_, co, dd, hh, ww = h_
                            for a in range(k[0]):
                                for b in range(k[1]):
                                    for c in range(k[2]):
                                        pd, ph, pw = dd + a - k[0] // 2, hh + b - k[1] // 2, ww + c - k[2] // 2
                                        assert 0 <= pd < D and 0 <= ph < H and (0 <= pw < W or planted == "border")
                                        ref[co, :, a, b, c] = np.sign(xq[n_, :, pd, ph, pw]) * np.inf if 0 <= pw < W else np.nan
                            assert not np.isfinite(ref[co]).any() and np.isfinite(ref[np.arange(Cout) != co]).all()
                            assert np.isnan(ref).any() == (planted == "border")
                        else:
                            ref = wgrad_ref(xq, gq, k)
                        gb = np.full((N, D, H, W, Cout + 24), np.nan, np.float32)
                        gb[..., 16:16 + Cout] = cl(g)
                        gd = bk.dev(encode(gb, gdt))
                        runs = [("plain", None)]
                        if nbw:
                            runs += [("ws", None), ("partial", None)]
                        for form, _ in runs:
                            dw = bk.dev(np.full((Cout, Cin) + k, 7.0, np.float32))
                            ws = bk.dev(np.full(max(nbw, 16) // 4, np.nan, np.float32))
                            if form == "plain":
                                assert plain(ctypes.byref(d), xd.ptr, gd.ptr, dw.ptr, 0, bk.stream) == 0
                            elif form == "ws":
                                assert with_ws(ctypes.byref(d), xd.ptr, gd.ptr, dw.ptr, 0, ws.ptr, nbw, bk.stream) == 0
                            else:
                                item = (_capi.WgradReduceItem * 1)()
                                assert bk.lib.step_conv_wgrad_partial(ctypes.byref(d), xd.ptr, gd.ptr, int(w16), dw.ptr, 0, ws.ptr, nbw, ctypes.byref(item[0]), bk.stream) == 0
                                assert bk.lib.step_wgrad_reduce_group(item, 1, bk.stream) == 0
                            got = dw.get()
                            what = ((N, Cin, Cout, D, H, W, k), dt, minpix, ldsopt, form, planted)
                            assert planted == "border" or not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
                            cg, cr = cls(got), cls(ref)
                            assert np.array_equal(cg, cr), (what, int((cg != cr).sum()), np.argwhere(cg != cr)[:4].tolist())
                            fin = cr == 0
                            err = float(np.abs(got[fin] - ref[fin]).max() / np.abs(ref[fin]).max())
                            assert err < 2e-5, (what, err)
    finally:
        _capi.set_option(bk.lib, "wgrad_minpix", 0)
        _capi.set_option(bk.lib, "wgrad16_lds", 1)


def plant_grad(g):
    """a copy of the incoming gradient [M, C] with a NaN of each sign, +inf and -inf in rows 1..4 (the forward tensors stay finite)"""
    g = np.array(g, np.float32, copy=True)
    g[1, 0], g[2, 1], g[3, 2], g[4, 3] = NAN_POS, NAN_NEG, INF, -INF
    return g


def case_nf_backward_elementwise(bk, golden):
    """Non-finite values in the INCOMING gradient only: step_act_grad (torch's ReLU backward SELECTS -- a masked element is 0 whatever the
    gradient holds, an unmasked one carries it on) and step_bn_train_backward (a non-finite gradient in a channel makes that channel's
    sums, hence its whole gz column, ggamma and gbeta non-finite -- in the class torch's backward gives element by element; the other
    channels are untouched), at the smallest shapes of
    case_act_grad / case_bn_train, against their references in double, by class."""
    rs = np.random.RandomState(47)
    # ---- step_act_grad
    M, C = 37, 24
    y = rs.randn(M, C).astype(np.float32)
    y[::5] = 0.0
    y[1, 0], y[2, 1], y[3, 2], y[4, 3] = 1.0, 0.5, 2.0, 0.25                 # the mask is open where plant_grad() plants
    gy = plant_grad(rs.randn(M, C).astype(np.float32))
    gy[0, 4], gy[5, 5] = NAN_POS, INF                                   # rows 0 and 5 are masked (y == 0): the select drops them
    scale = (1 + 0.3 * rs.randn(C)).astype(np.float32)
    z = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
    F.relu(z).backward(torch.from_numpy(gy.astype(np.float64)))
    assert np.array_equal(z.grad.numpy(), np.where(y > 0, gy.astype(np.float64), 0.0), equal_nan=True)      # torch selects
    for dt in DTS:
        yq = quantize(y, dt)
        for g_dt in (F32, dt):
            gq = quantize(gy, g_dt)
            for relu in (1, 0):
                with np.errstate(invalid="ignore"):
                    ref = gq.astype(np.float64) * scale[None, :]
                if relu:
                    ref = np.where(yq > 0, ref, 0.0)
                assert_planted_reference(ref, F32, ("act_grad", dt, relu))
                yd, gd, sd = bk.dev(encode(yq, dt)), bk.dev(encode(gq, g_dt)), bk.dev(scale)
                o32, oT = bk.dev(np.full((M, C), 9.0, np.float32)), bk.dev(encode(np.full((M, C), 9.0, np.float32), dt))
                assert bk.lib.step_act_grad(dt, yd.ptr, 0, g_dt, gd.ptr, 0, sd.ptr, M, C, relu, o32.ptr, oT.ptr, bk.stream) == 0
                check(o32.get(), ref, F32, ("act_grad fp32", dt, g_dt, relu))
                check(decode(oT.get(), dt), o32.get(), dt, ("act_grad storage", dt, g_dt, relu))
    # ---- step_bn_train_backward
    M, C = 300, 8
    zf = (rs.randn(M, C) * rs.uniform(0.5, 2.0, C) + rs.uniform(-3, 3, C)).astype(np.float32)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(np.float32), rs.uniform(-1, 1, C).astype(np.float32)
    g0 = rs.randn(M, C).astype(np.float32)
    for dt, gdt in ((F32, F32), (BF16, BF16), (F16, F32)):
        for relu in (1, 0):
            zq = quantize(zf, dt)
            Z, Y = bk.dev(encode(zq, dt)), bk.dev(np.zeros((M, C), NP_DT[dt]))
            G, Bt = bk.dev(gamma), bk.dev(beta)
            RM, RV = bk.dev(np.zeros(C, np.float32)), bk.dev(np.ones(C, np.float32))
            SM, SI = bk.dev(np.zeros(C, np.float32)), bk.dev(np.zeros(C, np.float32))
            wsb = bk.lib.step_bn_train_workspace_bytes(M, C)
            WS = bk.dev(np.full(wsb // 4 + 4, np.nan, np.float32))
            assert bk.lib.step_bn_train_forward(dt, Z.ptr, C, M, C, G.ptr, Bt.ptr, 1e-5, 0.1, RM.ptr, RV.ptr, SM.ptr, SI.ptr, relu, Y.ptr, C, WS.ptr, wsb,
                                                bk.stream) == 0
            ystored = decode(Y.get(), dt)
            assert np.isfinite(ystored).all()
            g = g0.copy()
            rows = np.flatnonzero(ystored[:, 0] > 0) if relu else np.arange(M)       # (a masked element drops its gradient: plant where the mask is open)
            g[rows[3], 0] = NAN_NEG
            rows2 = np.flatnonzero(ystored[:, 2] > 0) if relu else np.arange(M)
            g[rows2[5], 2] = INF
            gq = quantize(g, gdt)
            zt = torch.from_numpy(zq.astype(np.float64)).requires_grad_(True)
            gt, bt = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True), torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
            yr = F.batch_norm(zt.t().reshape(1, C, M), None, None, gt, bt, True, 0.1, 1e-5).reshape(C, M).t()
            gm = np.where(ystored > 0, gq.astype(np.float64), 0.0) if relu else gq.astype(np.float64)   # (the kernel masks with the STORED output)
            yr.backward(torch.from_numpy(gm))
            ref_gz, ref_gg, ref_gb = zt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()
            assert not np.isfinite(ref_gz[:, [0, 2]]).any() and np.isfinite(ref_gz[:, [1, 3, 4, 5, 6, 7]]).all()
            GY = bk.dev(encode(gq, gdt))
            GZ = bk.dev(np.zeros((M, C), NP_DT[dt]))
            GG, GB = bk.dev(np.zeros(C, np.float32)), bk.dev(np.zeros(C, np.float32))
            assert bk.lib.step_bn_train_backward(dt, Z.ptr, C, Y.ptr, C, gdt, GY.ptr, C, M, C, relu, G.ptr, SM.ptr, SI.ptr, GZ.ptr, GG.ptr, GB.ptr,
                                                 WS.ptr, wsb, bk.stream) == 0
            what = ("bn_train_backward", dt, gdt, relu)
            clean = [1, 3, 4, 5, 6, 7]
            fin = ref_gz[:, clean]
            check(decode(GZ.get(), dt), ref_gz, dt, what + ("gz",), bound=max(tol(dt), 2e-5) * max(1e-3, np.abs(fin).max()) * (4 if dt != F32 else 1))
            assert np.isnan(ref_gg[0]) and np.isnan(ref_gb[0]) and not np.isfinite(ref_gg[2]) and np.isposinf(ref_gb[2])
            for got, ref, nm in ((GG.get(), ref_gg, "ggamma"), (GB.get(), ref_gb, "gbeta")):
                check(got, ref, F32, what + (nm,), bound=(2e-2 if dt != F32 else 2e-4) * max(1.0, np.abs(ref[clean]).max()))


def case_nf_backward_gathers(bk, golden):
    """Non-finite values in the incoming gradient of the two gathering backward operators, forward tensors finite:
    step_roi_align_backward (fixed-order gather and atomics scatter, both layouts, adaptive and fixed sampling; `few` rois of
    case_roi_align_backward) against the C oracle's restatement of the reference's operator -- a cell is non-finite exactly where the
    oracle's is (a bilinear weight of exactly 0 times inf is NaN in both) -- and step_maxpool3d_tf_backward_gather at the shape of
    case_maxpool_backward against torch autograd in double: the gradient of a window goes to its winner and to nobody else."""
    import oracle
    rs = np.random.RandomState(53)
    rois = np.array([[0, 0, 0, 190, 140], [1, 33.3, 20.1, 120.7, 100.2], [1, -20, 100, 90, 250], [0, 50, 50, 50.5, 50.5]], np.float32)
    B, C, H, W = 2, 8, 9, 12
    K = rois.shape[0]
    g_in = rs.randn(K, C, 7, 7).astype(np.float32)
    g_in[0, 0, 3, 3], g_in[1, 1, 2, 4], g_in[0, 2, 4, 2], g_in[1, 3, 2, 2], g_in[0, 4, 1, 3], g_in[0, 4, 1, 4] = NAN_POS, NAN_NEG, INF, -INF, INF, -INF
    # ... and in bins on the map's border, whose samples are clamped to the last row / column: the reference's operator (and the oracle)
    # adds gradient x weight for both neighbours of a clamped sample, one weight being exactly 0 -- inf x 0 = NaN.  The gather keeps
    # those zero-weight terms (axis_weight, roi.hip), so both modes agree with the oracle cell by cell there too.
    g_edge = g_in.copy()
    g_edge[2, 2, 6, 0], g_edge[0, 5, 1, 6], g_edge[1, 6, 0, 6] = INF, -INF, NAN_NEG
    for mode in (_capi.ROI_BWD_GATHER, _capi.ROI_BWD_ATOMIC):
        for layout in (KC.NCHW, KC.NHWC):
            for sr in (0, 2):
                for g in (g_in, g_edge):
                    with np.errstate(invalid="ignore"):
                        ref = oracle.roi_align_backward(g, rois, (7, 7), 1 / 16., sr, (B, C, H, W))
                    assert_planted_reference(ref, F32, ("roi_align_backward", sr))
                    gg, r = bk.dev(g if layout == KC.NCHW else KC.nhwc(g)), bk.dev(rois)
                    gi = bk.dev(np.full((B, C, H, W) if layout == KC.NCHW else (B, H, W, C), 7.0, np.float32))
                    assert bk.lib.step_roi_align_backward(gg.ptr, layout, r.ptr, K, B, C, H, W, 7, 7, 1 / 16., sr, mode, gi.ptr, bk.stream) == 0
                    got = gi.get() if layout == KC.NCHW else KC.nchw(gi.get())
                    check(got, ref, F32, ("roi_align_backward", mode, layout, sr, g is g_edge), atol=1e-5)   # (1e-5: the existing bound, summation order)
    N, C, D, H, W = 2, 8, 5, 9, 7
    x = rs.randn(N, C, D, H, W).astype(np.float32)
    x[0] = np.maximum(x[0], 0)
    for k, s in KC.POOLS:
        pads = []
        for kk, ss in zip(reversed(k), reversed(s)):
            a = max(kk - ss, 0)
            pads += [a // 2, a - a // 2]
        for dt in DTS:
            xq = quantize(x, dt)
            xt = torch.from_numpy(xq.astype(np.float64)).requires_grad_(True)
            y = F.max_pool3d(F.pad(xt, pads), k, s, ceil_mode=True)
            gy, _ = plant(rs.randn(*y.shape).astype(np.float32), dt)
            gq = quantize(gy, dt)
            y.backward(torch.from_numpy(gq.astype(np.float64)))
            ref = xt.grad.numpy()
            assert_planted_reference(ref, F32, ("maxpool backward", k, dt), want=(0, 3))
            assert (cls(ref) == 1).any() or (cls(ref) == 2).any()
            Do, Ho, Wo = y.shape[2:]
            xe = bk.dev(encode(cl(xq), dt))
            ge = bk.dev(encode(np.ascontiguousarray(cl(gq)), dt))
            arg = bk.dev(np.full(N * Do * Ho * Wo * C, 250, np.uint8))
            go = bk.dev(np.full((N, D, H, W, C), 5.0, np.float32))
            assert bk.lib.step_maxpool3d_tf_backward_gather(dt, xe.ptr, N, D, H, W, C, C, 0, k[0], k[1], k[2], s[0], s[1], s[2], dt, ge.ptr, 0, go.ptr,
                                                            arg.ptr, bk.stream) == 0
            check(uncl(go.get()), ref, F32, ("maxpool backward", k, s, dt), atol=1e-6)


def case_nf_head_outputs(bk, golden):
    """step_head_outputs with a NaN and a +inf logit, and step_head_outputs_backward with non-finite incoming gradients (forward tensors
    finite), at the smallest shape of case_head_outputs (N = 7, Tl = T = 3) against the torch restatement of that case in double."""
    from step_amd.tube_math import encode_coef
    rs = np.random.RandomState(59)
    NC, T, N, Tl = 60, 3, 7, 3
    logits0 = (rs.randn(N * Tl, NC) * 2).astype(np.float32)
    reg = (rs.randn(N * Tl, 12) * 0.2).astype(np.float32)
    xy = rs.uniform(0, 250, (N, Tl, 2))
    tubes = np.concatenate([np.zeros((N, Tl, 1)), xy, xy + rs.uniform(20, 140, (N, Tl, 2))], 2).astype(np.float32)
    targets = np.zeros((N, 3, 6 + NC), np.float32)
    gxy = rs.uniform(0, 250, (N, 3, 2))
    targets[:, :, :4] = np.concatenate([gxy, gxy + rs.uniform(20, 140, (N, 3, 2))], 2)
    targets[:, :, 4] = 1
    targets[:, :, 5] = 1
    targets[:, :, 6:] = (rs.rand(N, 3, NC) < 0.1)
    targets[2, 1, 6 + 5], targets[2, 1, 6 + 6] = 0, 1                         # the +inf logits below meet a 0 and a 1 target

    def restate(logits, wc, w_loc, w_nbr):
        lt, rt = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True), torch.from_numpy(reg.astype(np.float64)).requires_grad_(True)
        tb, tg = torch.from_numpy(tubes).double(), torch.from_numpy(targets).double()
        gc = lt.reshape(N, Tl, NC).mean(1)
        r3 = rt.reshape(N, Tl, 12)
        ll = r3[..., 0:4]
        fl, la = ll + r3[..., 4:8], ll + r3[..., 8:12]
        ct, ft, ltg = tg[:, 1], tg[:, 0], tg[:, -1]
        m = ct[:, 4].reshape(-1, 1)
        l_cls = F.binary_cross_entropy_with_logits(gc, ct[:, 6:] * m, reduction="none")
        l_loc = F.smooth_l1_loss(ll[:, 1], encode_coef(ct[:, :4], tb[:, 1, 1:]), reduction="none").mean()
        ntgt = encode_coef(torch.cat([ft[:, :4], ltg[:, :4]], 0), torch.cat([tb[:, 1, 1:], tb[:, 1, 1:]], 0))
        l_nbr = F.smooth_l1_loss(torch.cat([fl[:, 1], la[:, 1]], 0), ntgt, reduction="none").mean()
        (l_cls * torch.from_numpy(wc.astype(np.float64))).sum().add(w_loc * l_loc).add(w_nbr * l_nbr).backward()
        return torch.sigmoid(gc).detach().numpy(), l_cls.detach().numpy(), lt.grad.numpy(), rt.grad.numpy()

    def run(logits, wc, w_loc, w_nbr):
        L_, R_, TB, TG = bk.dev(logits), bk.dev(reg), bk.dev(tubes), bk.dev(targets)
        prob, oll, ofl, ola = (bk.dev(np.zeros(sh, np.float32)) for sh in ((N, NC), (N, Tl, 4), (N, T, 4), (N, T, 4)))
        lc, lo_, ln = bk.dev(np.zeros((N, NC), np.float32)), bk.dev(np.zeros(1, np.float32)), bk.dev(np.zeros(1, np.float32))
        assert bk.lib.step_head_outputs(F32, L_.ptr, NC, R_.ptr, 12, N, Tl, T, NC, TB.ptr, TG.ptr, prob.ptr, oll.ptr, ofl.ptr, ola.ptr, lc.ptr, lo_.ptr, ln.ptr,
                                        bk.stream) == 0
        GL, GR = bk.dev(np.full((N * Tl, NC), 7, np.float32)), bk.dev(np.full((N * Tl, 12), 7, np.float32))
        gcl, glo, gnb = bk.dev(wc), bk.dev(np.array([w_loc], np.float32)), bk.dev(np.array([w_nbr], np.float32))
        assert bk.lib.step_head_outputs_backward(F32, L_.ptr, NC, R_.ptr, 12, N, Tl, T, NC, TB.ptr, TG.ptr, gcl.ptr, glo.ptr, gnb.ptr, GL.ptr, GR.ptr,
                                                 bk.stream) == 0
        return prob.get(), lc.get(), GL.get(), GR.get()

    wc0 = rs.randn(N, NC).astype(np.float32)
    # ---- forward: a NaN logit, a +inf logit under a 0 target (loss +inf) and under a 1 target (sigmoid 1, loss inf - inf)
    logits = logits0.copy()
    logits[1 * Tl + 0, 3], logits[2 * Tl + 1, 5], logits[2 * Tl + 2, 6] = NAN_NEG, INF, INF
    with np.errstate(invalid="ignore"):
        rprob, rlc, _, _ = restate(logits, wc0, 1.7, -0.6)
    assert np.isnan(rprob[1, 3]) and rprob[2, 5] == 1.0 and np.isposinf(rlc[2, 5]) and np.isnan(rlc[1, 3])
    prob, lc, _, _ = run(logits, wc0, 1.7, -0.6)
    check(prob, rprob, F32, "head_outputs: prob", atol=2e-6)
    check(lc, rlc, F32, "head_outputs: loss_cls", atol=5e-6)
    # a -inf logit: the kernel gives the LIMIT of the loss -- 0 under a 0 target, +inf under a 1 target -- where torch's (1 - t) * x +
    # max(-x, 0) + ... form gives inf - inf = NaN in both; a deliberate difference, pinned here
    logits = logits0.copy()
    logits[2 * Tl + 1, 5], logits[2 * Tl + 2, 6] = -INF, -INF
    with np.errstate(invalid="ignore"):
        rprob, rlc, _, _ = restate(logits, wc0, 1.7, -0.6)
    assert rprob[2, 5] == 0.0 and np.isnan(rlc[2, 5]) and np.isnan(rlc[2, 6])
    prob, lc, _, _ = run(logits, wc0, 1.7, -0.6)
    check(prob, rprob, F32, "head_outputs: prob, -inf logit", atol=2e-6)
    assert lc[2, 5] == 0.0 and np.isposinf(lc[2, 6]), (lc[2, 5], lc[2, 6])
    rest = np.ones(lc.shape, bool)
    rest[2, 5] = rest[2, 6] = False
    check(lc[rest], rlc[rest], F32, "head_outputs: loss_cls beside the -inf logits", atol=5e-6)
    # ---- backward: non-finite incoming gradients, finite logits
    wc = plant_grad(wc0)
    for w_loc, w_nbr in ((1.7, -0.6), (float("inf"), -0.6), (1.7, float("nan"))):
        with np.errstate(invalid="ignore"):
            _, _, rgl, rgr = restate(logits0, wc, w_loc, w_nbr)
        assert_planted_reference(rgl, F32, "head_outputs_backward: grad logits")
        _, _, gl, gr = run(logits0, wc, w_loc, w_nbr)
        check(gl, rgl, F32, ("head_outputs_backward: grad logits", w_loc, w_nbr), atol=1e-9)
        check(gr, rgr, F32, ("head_outputs_backward: grad reg", w_loc, w_nbr), atol=1e-9)


# ---- module cases (dev, golden) --------------------------------------------------------------------------------------------------------
def case_nf_basenet_forward(dev, golden):
    """The smallest BaseNet configuration of tests/module_cases.py (case_basenet_c1_golden's [1,8,3,112,112] clip) with ONE NaN voxel in a
    corner of the clip: stage by stage, wherever the oracle model (oracle.i3d_ref) has NaN, so has ours, and nowhere else -- in fp32 and
    in bf16 storage (which elements a NaN reaches is a matter of receptive fields, not of values)."""
    import step_amd
    from oracle import i3d_ref as R
    from tests import module_cases as MC

    net = MC.fill(step_amd.BaseNet(MC.cfg())).to(dev).eval()
    x = R.fill_tensor("golden.c1.images", (1, 8, 3, 112, 112), "image")
    x[0, 0, 1, 2, 3] = float("nan")
    with torch.no_grad():
        yo, ostages = R.basenet_forward(x, {k: v.detach().cpu() for k, v in net.state_dict().items()}, return_stages=True)
    assert len(ostages) == len(net.base_model)
    onan = [torch.isnan(s).numpy() for s in ostages]
    assert any(0 < m.mean() < 0.75 for m in onan), "the NaN stays local in at least one stage"
    assert np.isnan(yo.numpy()).any()
    for dt in (torch.float32, torch.bfloat16):
        stages = []          # (stage index, output): the stages that run inside a fused launch (stem + pool, 2b + 2c + pool in 16-bit storage) have none
        hooks = [m.register_forward_hook(lambda _m, _i, o, i=i: stages.append((i, o))) for i, m in enumerate(net.base_model)]
        with torch.no_grad():
            y = net(x.to(dev).to(dt))
        for h in hooks:
            h.remove()
        assert len(stages) >= len(onan) - 5 and (dt != torch.float32 or len(stages) == len(onan))
        for i, s in stages:
            m = onan[i]
            a = MC.np_(s.permute(0, 4, 1, 2, 3))
            assert not np.isinf(a).any(), (dt, i)
            assert np.array_equal(np.isnan(a), m), (dt, i, int(np.isnan(a).sum()), int(m.sum()))
        assert np.array_equal(np.isnan(MC.np_(y)), np.isnan(yo.numpy())), dt


def case_nf_fp16_step_is_skipped(dev, golden):
    """case_fp16_training_step_loss_scaling's setup at scale 2^12 with a non-finite value in the pooled features (a forward overflow in the
    backbone): once one NaN, once a +inf / -inf pair in two channels of a pixel.  The NaN must ARRIVE in the flat gradient arena -- an
    fmaxf ReLU turned it into 0, the loss came out finite and the step was taken -- so FlatAdam.step(scaler=...) leaves parameters, both
    moments and the step count bit-identical and halves the scale; the next clean step goes through."""
    import step_amd
    from oracle import i3d_ref as R
    from tests import module_cases as MC

    g = golden("head_golden")
    pf = R.fill_tensor("golden.det.pooled3", (2, 3, 832, 7, 7), "feat").to(dev).half()
    cx = R.fill_tensor("golden.det.ctx3", (2, 1024, 3, 1, 1), "feat").to(dev).half()
    tubes, targets = torch.from_numpy(g["loss_tubes"]).to(dev), torch.from_numpy(g["loss_targets"]).to(dev)
    net = MC.fill(step_amd.TwoBranchNet(MC.cfg()), "det0.").to(dev)
    net.set_device(dev)
    net.train()
    opt = step_amd.FlatAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4, capturable=True)

    def loss_of(feat):
        o = net(feat, context_feat=cx, tubes=tubes, targets=targets)
        return o[4].mean() + 5.0 * o[5].mean() + o[6].mean()

    sc = step_amd.LossScaler(torch.device(dev), init_scale=2.0 ** 12, growth_interval=1000)
    sc.scale_loss(loss_of(pf)).backward()
    assert bool(torch.isfinite(opt.flat_grad).all())
    opt.step(scaler=sc, zero_grad=True)
    assert opt.step_count == 1 and sc.scale == 4096.0
    for kind in ("nan", "inf pair"):
        bad = pf.clone()
        if kind == "nan":
            bad[1, 1, 400, 3, 3] = float("nan")
        else:
            bad[0, 2, 17, 5, 2], bad[0, 2, 600, 5, 2] = float("inf"), float("-inf")
        scale0, steps0 = sc.scale, opt.step_count
        before = [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
        sc.scale_loss(loss_of(bad)).backward()
        assert not bool(torch.isfinite(opt.flat_grad).all()), (kind, "the non-finite value never reached the gradient arena")
        opt.step(scaler=sc, zero_grad=True)
        assert opt.step_count == steps0, kind
        for a, b in zip(before, (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)):
            assert torch.equal(a, b), kind
        assert sc.scale == scale0 / 2 and not bool(opt.flat_grad.any()), kind
        sc.scale_loss(loss_of(pf)).backward()
        assert bool(torch.isfinite(opt.flat_grad).all())
        opt.step(scaler=sc, zero_grad=True)
        assert opt.step_count == steps0 + 1 and not torch.equal(opt.flat_param, before[0]) and bool(torch.isfinite(opt.flat_param).all()), kind
        assert sc.scale == scale0 / 2, kind


KERNEL_CASES = ["case_nf_conv_forms", "case_nf_conv_fused_forms", "case_nf_stem", "case_nf_maxpool", "case_nf_bn_train", "case_nf_wgrad_sliced_operands", "case_nf_backward_elementwise", "case_nf_backward_gathers", "case_nf_head_outputs"]
MODULE_CASES = ["case_nf_basenet_forward", "case_nf_fp16_step_is_skipped"]
CPU_MODULE_CASES = ["case_nf_basenet_forward"]            # (the fp16 training step is a GPU case, as case_fp16_training_step_loss_scaling)
