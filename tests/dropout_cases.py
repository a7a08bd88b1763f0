"""Cases for the device-side dropout (step_dropout_forward / _backward, step_rng_words, step_amd.Dropout, step_amd.rng), driven on the
host interpreter by tests/test_emul_dropout.py and on the real library by tests/test_gpu_dropout.py.

The reference of every kernel comparison is the numpy restatement of the stream below (integer arithmetic on uint64 arrays, written
from the definition in include/step_amd.h, checked here against Random123's published Philox4x32-10 vectors): masks and values are
compared for EQUALITY -- the pass is one generator draw, one comparison and one rounded multiply per element, there is nothing to
tolerate.  The statistical bounds (5 standard deviations of a binomial share) are first asserted of the restatement itself.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import numpy as np
import torch

import step_amd
from step_amd import _capi

F32, BF16, F16 = _capi.F32, _capi.BF16, _capi.F16
u64 = np.uint64
M32 = u64(0xFFFFFFFF)

# Random123's known-answer vectors for Philox4x32-10: (counter, key, words)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

SIZES = [1, 31, 32, 33, 4 * 64 * 32 + 5, 3 * 12544]          # lone tail; word boundary (under, at, over); waves of a block + tail; the head's row
PS = [0.3, 0.5]
# (seed, offset): small; seed and offset above 2^32; the top bit set
STATES = [(0x1234, 0), (0x1_0000_0007, 0x2_0000_0003), (0xF00D_0000_0000_0001, 0xFFFF_FFFF)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def philox_words(seed, offset, first_blk, n_blk):
    """words [n_blk, 4] (uint64 holding 32-bit values) of blocks first_blk .. first_blk + n_blk - 1 at (seed, offset)"""
    blk = (np.arange(n_blk, dtype=u64) + u64(first_blk & 0xFFFFFFFFFFFFFFFF))         # wraps modulo 2^64 like the device's counter
    c0, c1 = blk & M32, blk >> u64(32)
    c2 = np.full(n_blk, offset & 0xFFFFFFFF, u64)
    c3 = np.full(n_blk, (offset >> 32) & 0xFFFFFFFF, u64)
    k0, k1 = u64(seed & 0xFFFFFFFF), u64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2                        # 32 x 32 -> 64, exact in uint64
        c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> u64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + u64(0x9E3779B9)) & M32, (k1 + u64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], 1)


def thr_of(p):
    return int(np.floor(np.float64(p) * 4294967296.0))


def scale_of(p):
    return np.float32(0.0) if p == 1 else np.float32(1.0 / (1.0 - p))


def keep_of(seed, offset, n, p):
    """bool [n]: element e is kept iff word (e & 3) of block (e >> 2) >= floor(p * 2^32)"""
    w = philox_words(seed, offset, 0, (n + 3) // 4).reshape(-1)[:n]
    return w >= u64(thr_of(p))


def pack_mask(keep):
    """bool [n] -> uint32 [ceil(n / 32)], bit e & 31 of word e >> 5; high bits of the last word 0"""
    n = len(keep)
    b = np.zeros(((n + 31) // 32) * 32, np.uint8)
    b[:n] = keep
    return np.packbits(b.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)


def unpack_mask(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def to_bf16_bits(x):
    """float32 -> bfloat16 bits, round to nearest even (finite values and infinities)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(u64)
    return ((u + u64(0x7FFF) + ((u >> u64(16)) & u64(1))) >> u64(16)).astype(np.uint16)


def from_bf16_bits(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def encode(x32, dt):
    """float32 values -> the array handed to the backend (fp16 / bf16 travel as uint16 bit patterns)"""
    if dt == F32:
        return np.ascontiguousarray(x32, np.float32)
    return to_bf16_bits(x32) if dt == BF16 else np.asarray(x32, np.float32).astype(np.float16).view(np.uint16)


def decode(a, dt):
    if dt == F32:
        return a
    return from_bf16_bits(a) if dt == BF16 else a.view(np.float16).astype(np.float32)


def expect(xbits, keep, p, dt):
    """where(keep, round_to_dtype(float(x) * float32(scale)), +0) as the backend's array type"""
    with np.errstate(invalid="ignore", over="ignore"):
        prod = decode(xbits, dt) * scale_of(p)                                     # one float32 multiply
    return encode(np.where(keep, prod, np.float32(0.0)).astype(np.float32), dt)


def _state(bk, seed, offset):
    return bk.dev(np.array([seed, offset], u64).view(np.int64))


def _read_state(st):
    s = st.get().view(u64)
    return int(s[0]), int(s[1])


def _inputs(n, keep, dt, rs):
    """quantised normal values with NaN / +-inf planted at DROPPED positions (a dropped element is +0 by selection)"""
    x = rs.randn(n).astype(np.float32)
    x[rs.rand(n) < 0.05] *= -0.0                                                  # a few signed zeros
    dropped = np.flatnonzero(~keep)
    if len(dropped):
        pick = dropped[rs.permutation(len(dropped))[:9]]
        x[pick[0::3]] = np.nan
        x[pick[1::3]] = np.inf
        x[pick[2::3]] = -np.inf
    return encode(x, dt)


def _forward(bk, dt, xbits, p, st, in_place=False):
    n = len(xbits)
    X = bk.dev(xbits.copy())
    Y = X if in_place else bk.dev(np.zeros_like(xbits))
    Mk = bk.dev(np.full((n + 31) // 32, 0xA5A5A5A5, np.uint32).view(np.int32))
    assert bk.lib.step_dropout_forward(dt, X.ptr, Y.ptr, Mk.ptr, n, p, st.ptr, bk.stream) == 0
    return Y.get().copy(), Mk.get().view(np.uint32).copy(), X.get().copy()


# ---- kernel cases --------------------------------------------------------------------------------------------------------------
def case_rng_known_answers(bk, golden):
    """step_rng_words reproduces Random123's three Philox4x32-10 vectors (and so does the restatement the other cases compare with);
    a run of blocks that crosses 2^32 in the block index carries into the counter's second word; the state is left as it was."""
    for ctr, key, want in KAT:
        seed, offset, first = key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, ctr[0] | ctr[1] << 32
        assert tuple(int(v) for v in philox_words(seed, offset, first, 1)[0]) == want
        st = _state(bk, seed, offset)
        out = bk.dev(np.zeros(4, np.int32))
        assert bk.lib.step_rng_words(st.ptr, first, 1, out.ptr, bk.stream) == 0
        got = tuple(int(v) for v in out.get().view(np.uint32))
        assert got == want, (["%08x" % v for v in got], ["%08x" % v for v in want])
        assert _read_state(st) == (seed, offset)
    seed, offset, first, nb = STATES[1][0], STATES[1][1], (1 << 32) - 300, 1000   # 4 grid blocks of 256 threads, the last one partial
    st = _state(bk, seed, offset)
    out = bk.dev(np.zeros(4 * nb, np.int32))
    assert bk.lib.step_rng_words(st.ptr, first, nb, out.ptr, bk.stream) == 0
    assert np.array_equal(out.get().view(np.uint32).reshape(nb, 4).astype(u64), philox_words(seed, offset, first, nb))
    assert _read_state(st) == (seed, offset)


def _matches(bk, dt):
    rs = np.random.RandomState(17 + dt)
    for k, n in enumerate(SIZES):
        for j, p in enumerate(PS):
            seed, offset = STATES[(k + j) % len(STATES)]
            keep = keep_of(seed, offset, n, p)
            xbits = _inputs(n, keep, dt, rs)
            want_y, want_m = expect(xbits, keep, p, dt), pack_mask(keep)
            st = _state(bk, seed, offset)
            y, m, x_after = _forward(bk, dt, xbits, p, st)
            assert np.array_equal(m, want_m), (n, p, "mask")
            assert n % 32 == 0 or (int(m[-1]) >> (n % 32)) == 0, (n, "tail bits")
            assert np.array_equal(y.view(np.uint8), want_y.view(np.uint8)), (n, p, "values")                 # bit patterns: +0 where dropped, NaN-free
            assert np.array_equal(x_after.view(np.uint8), xbits.view(np.uint8))                              # the input is read only
            assert _read_state(st) == (seed, (offset + 1) & 0xFFFFFFFFFFFFFFFF)
            st2 = _state(bk, seed, offset)
            y2, m2, _ = _forward(bk, dt, xbits, p, st2, in_place=True)
            assert np.array_equal(m2, want_m) and np.array_equal(y2.view(np.uint8), want_y.view(np.uint8)), (n, p, "in place")


def case_dropout_matches_restatement_f32(bk, golden):
    _matches(bk, F32)


def case_dropout_matches_restatement_bf16(bk, golden):
    _matches(bk, BF16)


def case_dropout_matches_restatement_f16(bk, golden):
    _matches(bk, F16)


_matches.__doc__ = """step_dropout_forward against the numpy restatement: n in SIZES x p in {0.3, 0.5} over three states (a seed and an offset above
    2^32 among them), NaN / inf planted at dropped positions.  Mask words bit-equal, the tail word's high bits 0, y bit-equal to
    where(keep, x * float32(scale), +0) -- rounded to nearest even for the 16-bit types --, the offset one further, and the same again
    with y == x."""
for _f in (case_dropout_matches_restatement_f32, case_dropout_matches_restatement_bf16, case_dropout_matches_restatement_f16):
    _f.__doc__ = _matches.__doc__


def case_dropout_misaligned(bk, golden):
    """Tensors that start 4 bytes into a 16-byte line (a view of a wider buffer) take the element-by-element path: same stream, same
    result, nothing written in front of or behind the view."""
    import ctypes
    n, p, (seed, offset) = 2 * 64 * 32 + 7, 0.3, STATES[1]
    keep = keep_of(seed, offset, n, p)
    rs = np.random.RandomState(3)
    x = rs.randn(n + 2).astype(np.float32)
    X, Y = bk.dev(x.copy()), bk.dev(np.full(n + 2, 7.0, np.float32))
    Mk = bk.dev(np.zeros((n + 31) // 32, np.int32))
    st = _state(bk, seed, offset)
    addr = lambda b: (b.ptr.value if isinstance(b.ptr, ctypes.c_void_p) else int(b.ptr)) + 4
    assert bk.lib.step_dropout_forward(F32, ctypes.c_void_p(addr(X)), ctypes.c_void_p(addr(Y)), Mk.ptr, n, p, st.ptr, bk.stream) == 0
    y = Y.get()
    assert y[0] == 7.0 and y[-1] == 7.0
    assert np.array_equal(y[1:-1].view(np.uint32), expect(x[1:-1], keep, p, F32).view(np.uint32))
    assert np.array_equal(Mk.get().view(np.uint32), pack_mask(keep))


def case_dropout_edges(bk, golden):
    """p = 0: the identity, every valid mask bit set (the tail word's high bits still 0); p = 1: every element +0 (sign bit clear, also
    for negative, NaN and inf inputs), mask all zeros.  p outside [0, 1] and a bad dtype are refused with nothing written and the offset
    where it was; n = 0 succeeds and still counts as a call."""
    rs = np.random.RandomState(1)
    n = 4 * 64 * 32 + 5
    for dt in (F32, BF16, F16):
        x = rs.randn(n).astype(np.float32)
        x[:3] = [np.nan, np.inf, -np.inf]
        xbits = encode(x, dt)
        st = _state(bk, 9, 5)
        y, m, _ = _forward(bk, dt, xbits, 0.0, st)
        assert np.array_equal(y.view(np.uint8), xbits.view(np.uint8))
        assert np.array_equal(m, pack_mask(np.ones(n, bool))) and int(m[-1]) == (1 << (n % 32)) - 1
        y, m, _ = _forward(bk, dt, xbits, 1.0, st)
        assert not y.view(np.uint8).any() and not m.any()                          # all bits clear: +0, never -0
        assert _read_state(st) == (9, 7)
        Y, Mk = bk.dev(np.full_like(xbits, 3)), bk.dev(np.full((n + 31) // 32, 5, np.int32))
        X = bk.dev(xbits.copy())
        for bad_p in (-0.1, 1.5, float("nan")):
            assert bk.lib.step_dropout_forward(dt, X.ptr, Y.ptr, Mk.ptr, n, bad_p, st.ptr, bk.stream) < 0
            assert bk.lib.step_dropout_backward(dt, X.ptr, Y.ptr, Mk.ptr, n, bad_p, bk.stream) < 0
        assert bk.lib.step_dropout_forward(7, X.ptr, Y.ptr, Mk.ptr, n, 0.5, st.ptr, bk.stream) < 0
        assert bk.lib.step_dropout_forward(dt, X.ptr, Y.ptr, Mk.ptr, -1, 0.5, st.ptr, bk.stream) < 0
        assert bk.lib.step_dropout_forward(dt, X.ptr, Y.ptr, Mk.ptr, n, 0.5, None, bk.stream) < 0
        assert np.all(Y.get() == 3) and np.all(Mk.get() == 5) and _read_state(st) == (9, 7)
        assert bk.lib.step_dropout_forward(dt, None, None, None, 0, 0.5, st.ptr, bk.stream) == 0
        assert _read_state(st) == (9, 8)


def case_dropout_state(bk, golden):
    """K calls move the offset from start to start + K; two successive calls draw different masks, each the restatement's at its own
    offset; re-seeding (writing {seed, start} back) reproduces the first mask; step_rng_words does not move the state."""
    n, p, seed, start, K = 4 * 64 * 32 + 5, 0.3, 0x1_0000_0007, 0xFFFF_FFFE, 4    # the offset crosses 2^32 on the way
    xbits = np.random.RandomState(2).randn(n).astype(np.float32)
    st = _state(bk, seed, start)
    masks = []
    for k in range(K):
        _, m, _ = _forward(bk, F32, xbits, p, st)
        masks.append(m)
        assert _read_state(st) == (seed, start + k + 1)
        assert np.array_equal(m, pack_mask(keep_of(seed, start + k, n, p))), k
    assert not np.array_equal(masks[0], masks[1])
    out = bk.dev(np.zeros(8, np.int32))
    assert bk.lib.step_rng_words(st.ptr, 0, 2, out.ptr, bk.stream) == 0
    assert _read_state(st) == (seed, start + K)
    st = _state(bk, seed, start)
    _, m, _ = _forward(bk, F32, xbits, p, st)
    assert np.array_equal(m, masks[0])


def _share_bounds(keep_a, keep_b, p):
    """the two statistics and their 5-sigma bounds: (kept share, its expectation, bound), (share kept by both, expectation, bound)"""
    n = len(keep_a)
    q = 1.0 - thr_of(p) / 4294967296.0
    s1, s2 = float(keep_a.mean()), float((keep_a & keep_b).mean())
    return (s1, q, 5.0 * np.sqrt(q * (1 - q) / n)), (s2, q * q, 5.0 * np.sqrt(q * q * (1 - q * q) / n))


def case_dropout_statistics(bk, golden):
    """Deterministic: seed 2024, n = 2^20, p = 0.3, two consecutive offsets.  The kept share lies within 5 standard deviations
    sqrt(q (1 - q) / n) of q = 1 - thr / 2^32, and the share kept by BOTH offsets within 5 standard deviations of q^2 (independent
    masks: a binomial share with probability q^2).  The restatement is held to the same bounds first."""
    n, p, seed = 1 << 20, 0.3, 2024
    ra, rb = keep_of(seed, 0, n, p), keep_of(seed, 1, n, p)
    for got, want, bound in _share_bounds(ra, rb, p):
        assert abs(got - want) <= bound, ("restatement", got, want, bound)
    xbits = encode(np.ones(n, np.float32), BF16)
    st = _state(bk, seed, 0)
    _, ma, _ = _forward(bk, BF16, xbits, p, st)
    _, mb, _ = _forward(bk, BF16, xbits, p, st)
    ka, kb = unpack_mask(ma, n), unpack_mask(mb, n)
    for got, want, bound in _share_bounds(ka, kb, p):
        print("dropout statistics %s: share %.6f, expected %.6f, 5 sigma %.6f" % (bk.name, got, want, bound))
        assert abs(got - want) <= bound, (got, want, bound)


def case_dropout_backward(bk, golden):
    """step_dropout_backward with a hand-made mask (alternating runs, not a mask the generator would draw): gx bit-equal to
    where(bit, round(float(gy) * scale), +0) in the three dtypes, inf / NaN under a clear bit become +0, in place (gx == gy) the same.
    The call takes no generator: a forward pass on some state between two backward calls changes nothing."""
    n = 4 * 64 * 32 + 5
    rs = np.random.RandomState(4)
    keep = ((np.arange(n) // 3) % 2 == 0) ^ (rs.rand(n) < 0.1)
    words = pack_mask(keep)
    for dt in (F32, BF16, F16):
        for p in PS:
            g = rs.randn(n).astype(np.float32)
            g[rs.rand(n) < 0.05] *= -0.0                                          # signed zeros: a kept -0 stays -0
            clear = np.flatnonzero(~keep)
            g[clear[:3]] = [np.nan, np.inf, -np.inf]
            gbits = encode(g, dt)
            want = expect(gbits, keep, p, dt)
            GY, GX, Mk = bk.dev(gbits.copy()), bk.dev(np.zeros_like(gbits)), bk.dev(words.view(np.int32).copy())
            assert bk.lib.step_dropout_backward(dt, GY.ptr, GX.ptr, Mk.ptr, n, p, bk.stream) == 0
            assert np.array_equal(GX.get().view(np.uint8), want.view(np.uint8)), (dt, p)
            st = _state(bk, 77, 3)
            _forward(bk, F32, np.ones(64, np.float32), 0.5, st)
            assert bk.lib.step_dropout_backward(dt, GY.ptr, GY.ptr, Mk.ptr, n, p, bk.stream) == 0
            assert np.array_equal(GY.get().view(np.uint8), want.view(np.uint8)), (dt, p, "in place")
            assert np.array_equal(Mk.get().view(np.uint32), words)


def big_dropout_full_size(bk, golden):
    """One call site of the C4 step at 8 clips x 15 tubes x 9 frames: 1080 x 12544 bf16 elements against the restatement, mask and
    values equal."""
    n, p, (seed, offset) = 1080 * 12544, 0.3, STATES[1]
    keep = keep_of(seed, offset, n, p)
    xbits = to_bf16_bits(np.random.RandomState(8).randn(n).astype(np.float32))
    st = _state(bk, seed, offset)
    y, m, _ = _forward(bk, BF16, xbits, p, st)
    assert np.array_equal(m, pack_mask(keep))
    assert np.array_equal(y, expect(xbits, keep, p, BF16))
    assert _read_state(st) == (seed, offset + 1)


KERNEL_CASES = ["case_rng_known_answers", "case_dropout_matches_restatement_f32", "case_dropout_matches_restatement_bf16",
                "case_dropout_matches_restatement_f16", "case_dropout_misaligned", "case_dropout_edges", "case_dropout_state",
                "case_dropout_statistics", "case_dropout_backward"]
KERNEL_GPU_ONLY = ["big_dropout_full_size"]


# ---- module cases --------------------------------------------------------------------------------------------------------------
def np_(t):
    return t.detach().float().cpu().contiguous().numpy()


class _Recorder:
    """wraps step_amd.ops.dropout for the length of a `with`: keeps (mask words, element count, p) of every call"""

    def __enter__(self):
        from step_amd import ops
        self.ops, self.orig, self.calls = ops, ops.dropout, []

        def wrapped(x, p, rng=None, out=None):
            y, mask = self.orig(x, p, rng, out=out)
            self.calls.append((mask, x.numel(), p))
            return y, mask
        ops.dropout = wrapped
        return self

    def __exit__(self, *exc):
        self.ops.dropout = self.orig
        return False


def _keep_tensor(mask, n, shape, dev):
    words = mask.detach().cpu().numpy().view(np.uint32)
    return torch.from_numpy(unpack_mask(words, n)).reshape(shape).to(dev)


def case_dropout_module(dev, golden):
    """step_amd.Dropout: nn.Dropout's constructor, `p`, no parameters or buffers; eval mode and p = 0 hand the input back with the
    generator's offset where it was; in train mode y.sum().backward() leaves x.grad == unpack(mask) * scale, the mask being the
    restatement's at the generator's (seed, offset); inplace=True writes into the input; ops.dropout takes a generator of the caller's own; the default generator follows
    step_amd.manual_seed and get_state / set_state round-trip."""
    step_amd.manual_seed(0x1_0000_0005)
    g = step_amd.rng.default(dev)
    assert g.get_state() == (0x1_0000_0005, 0) and g.offset() == 0
    d = step_amd.Dropout(0.3)
    assert isinstance(d, torch.nn.Module) and d.p == 0.3 and not list(d.parameters()) and not list(d.buffers()) and not d.state_dict()
    for bad in (-0.1, 1.1):
        try:
            step_amd.Dropout(bad)
        except ValueError:
            continue
        raise AssertionError("Dropout accepted p = %r" % bad)
    x = torch.randn(5, 41, 7, device=dev, requires_grad=True)
    d.eval()
    assert d(x) is x
    z = step_amd.Dropout(0.0).train()
    assert z(x) is x
    assert g.offset() == 0
    d.train()
    with _Recorder() as rec:
        y = d(x)
    y.sum().backward()
    assert g.offset() == 1 and len(rec.calls) == 1
    n = x.numel()
    keep = keep_of(0x1_0000_0005, 0, n, 0.3)
    assert np.array_equal(rec.calls[0][0].cpu().numpy().view(np.uint32), pack_mask(keep))
    want = np.where(keep, scale_of(0.3), np.float32(0)).reshape(x.shape)
    assert np.array_equal(np_(x.grad), want)
    assert np.array_equal(np_(y), np.where(keep.reshape(x.shape), np_(x) * scale_of(0.3), np.float32(0)))
    # in place: the input tensor itself is the output
    xi = x.detach().clone()
    assert step_amd.Dropout(0.3, inplace=True).train()(xi) is xi and g.offset() == 2
    assert np.array_equal(np_(xi), np.where(keep_of(0x1_0000_0005, 1, n, 0.3).reshape(x.shape), np_(x) * scale_of(0.3), np.float32(0)))
    # ops.dropout with a generator of the caller's own; the default one does not move
    from step_amd import ops
    mine = step_amd.DeviceRNG(dev, seed=77)
    y2, _ = ops.dropout(x.detach(), 0.5, mine)
    assert mine.offset() == 1 and g.offset() == 2
    assert np.array_equal(np_(y2) != 0, keep_of(77, 0, n, 0.5).reshape(x.shape) & (np_(x) != 0))
    # checkpointing: the state travels as two host integers
    mine.set_state((0xF00D_0000_0000_0001, 0x2_0000_0003))
    assert mine.get_state() == (0xF00D_0000_0000_0001, 0x2_0000_0003)
    step_amd.manual_seed(5)
    assert g.get_state() == (5, 0) and mine.get_state()[0] == 0xF00D_0000_0000_0001        # only the default generators follow manual_seed


class _ReplayDropout(torch.nn.Module):
    """TEST ONLY: stands in for head.dropout and multiplies by recorded masks and the scale, in call order, with torch operators"""

    def __init__(self, keeps, p):
        super().__init__()
        self.keeps, self.scale, self.k = keeps, float(scale_of(p)), 0

    def forward(self, x):
        keep = self.keeps[self.k].reshape(x.shape)
        self.k += 1
        return torch.where(keep, x * self.scale, torch.zeros((), dtype=x.dtype, device=x.device))


def _head_inputs(dev, golden):
    from oracle import i3d_ref as R
    g = golden("head_golden")
    pf = R.fill_tensor("golden.det.pooled3", (2, 3, 832, 7, 7), "feat").to(dev)
    cx = R.fill_tensor("golden.det.ctx3", (2, 1024, 3, 1, 1), "feat").to(dev)
    return pf, cx, torch.from_numpy(g["loss_tubes"]).to(dev), torch.from_numpy(g["loss_targets"]).to(dev)


def _head(dev, p, **kw):
    from tests.module_cases import cfg, fill
    cls_only = kw.pop("cls_only", False)
    net = fill(step_amd.TwoBranchNet(cfg(dropout=p, **kw), cls_only=cls_only), "det0.").to(dev)
    net.set_device(dev)
    return net


def _loss_and_grads(net, pf, cx, tubes, targets):
    for q in net.parameters():
        q.grad = None
    o = net(pf, context_feat=cx, tubes=tubes, targets=targets)
    loss = o[4].mean() + 5.0 * o[5].mean() + o[6].mean()
    loss.backward()
    return [np_(o[i]) for i in (4, 5, 6)], {k: np_(q.grad) for k, q in net.named_parameters() if q.grad is not None}


def case_head_dropout_eval_and_offsets(dev, golden):
    """TwoBranchNet with cfg.dropout = 0.3 (fp32, the head shapes of tests/module_cases.py): its `dropout` is step_amd.Dropout and the
    state_dict keys are those of a dropout = 0 net; (a) eval-mode outputs are bit-equal to the dropout = 0 net with the same weights and
    leave the generator alone; (b) one train-mode forward advances the offset by 2 with no_context and by 2 with cls_only (by 3 in the
    default configuration: case_head_dropout_replay_and_seeds)."""
    pf, cx, tubes, targets = _head_inputs(dev, golden)
    step_amd.manual_seed(11)
    g = step_amd.rng.default(dev)
    net, net0 = _head(dev, 0.3), _head(dev, 0.0)
    assert isinstance(net.dropout, step_amd.Dropout) and net.dropout.p == 0.3
    assert list(net.state_dict()) == list(net0.state_dict())
    net.eval()
    net0.eval()
    with torch.no_grad():
        a, b = net(pf, context_feat=cx), net0(pf, context_feat=cx)
    for u, v in zip(a, b):
        assert np.array_equal(np_(u), np_(v))
    assert g.offset() == 0
    # (the default configuration's 3 is asserted in case_head_dropout_replay_and_seeds, which runs that forward anyway)
    for want, kw, ctx in ((2, {"no_context": True}, None), (2, {"cls_only": True}, cx)):
        h = _head(dev, 0.3, **kw)
        h.train()
        before = g.offset()
        with torch.no_grad():
            h(pf, context_feat=ctx, tubes=tubes, targets=targets)
        assert g.offset() - before == want, (kw, g.offset() - before)


def case_head_dropout_replay_and_seeds(dev, golden):
    """(c) Replay parity: the three masks of a train-mode forward + backward are recorded by wrapping ops.dropout, then the same head
    runs again with head.dropout replaced by a torch module that multiplies by the recorded masks and the scale: the three losses and
    every parameter gradient are equal (np.array_equal) -- the kernels' forward AND backward are what torch computes from the same
    mask.  (d) The same seed again gives identical losses, another seed different ones."""
    pf, cx, tubes, targets = _head_inputs(dev, golden)
    net = _head(dev, 0.3).train()
    step_amd.manual_seed(21)
    with _Recorder() as rec:
        losses, grads = _loss_and_grads(net, pf, cx, tubes, targets)
    assert len(rec.calls) == 3 and step_amd.rng.default(dev).offset() == 3
    keeps = [_keep_tensor(m, n, (n,), dev) for m, n, _ in rec.calls]
    share = [float(k.float().mean()) for k in keeps]
    assert all(0.6 < s < 0.8 for s in share), share                               # really dropping: ~70 % kept at each site
    device_dropout = net.dropout
    net.dropout = _ReplayDropout(keeps, 0.3)
    losses_t, grads_t = _loss_and_grads(net, pf, cx, tubes, targets)
    net.dropout = device_dropout
    assert step_amd.rng.default(dev).offset() == 3                                # the stand-in drew nothing
    for a, b in zip(losses, losses_t):
        assert np.array_equal(a, b), (a, b)
    assert sorted(grads) == sorted(grads_t) and len(grads) > 10
    for k in grads:
        assert np.array_equal(grads[k], grads_t[k]), k
    # (d)
    step_amd.manual_seed(21)
    o = net(pf, context_feat=cx, tubes=tubes, targets=targets)                    # (grad mode as above: the no-grad forward takes other launches)
    for a, i in zip(losses, (4, 5, 6)):
        assert np.array_equal(a, np_(o[i]))
    step_amd.manual_seed(22)
    o = net(pf, context_feat=cx, tubes=tubes, targets=targets)
    assert any(not np.array_equal(a, np_(o[i])) for a, i in zip(losses, (4, 5, 6)))


MODULE_CASES = ["case_dropout_module", "case_head_dropout_eval_and_offsets", "case_head_dropout_replay_and_seeds"]
