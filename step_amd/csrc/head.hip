// step_amd/csrc/head.hip -- everything TwoBranchNet.forward does AFTER its last two GEMMs (models/two_branch.py:246-333), forward and
// backward, as one launch each:
//   global_class = mean over the tube's frames of the class logits (:247-249), global_prob = sigmoid (:341)
//   local_loc = the regressor's first 4 columns, first_loc / last_loc = local_loc + the neighbour regressors on the first / last
//   chunk (:262-270), center / first / last predictions (:271-273)
//   loss_global_cls = BCE-with-logits against the centre frame's labels, masked (:281-299)
//   loss_local_loc / loss_neighbor_loc = masked-mean smooth-L1 against encode_coef targets (:301-333; utils/tube_utils.py:127-157)
// In the reference (and in this package until round 4) that is ~60 element-wise torch kernels per head and step and as many again
// in backward -- ~350 launches of a 1300-launch training step, every one a few microseconds of latency on a few hundred values.
// The tensors are tiny (N <= a few hundred tubes, 60 classes, 12 regressor columns): ONE 256-thread workgroup does it all, with
// fixed-order reductions (bit-reproducible).  The reference's `if mask.sum():` host branches are taken on the device: an all-zero
// mask gives exactly zero losses and zero gradients (heads.py SYNC_FREE_LOSSES documents the one visible difference in shape).
#include "common.h"
#include <cmath>

namespace step {

struct HeadParams {
    const void* logits; int lcs;          // [N*Tl rows, >= NC] activation dtype, row stride lcs elements
    const void* reg; int rcs;             // [N*Tl rows, >= 12]
    int N, Tl, T, NC;
    int c_first, c_mid, c_last;           // frame of the first / middle / last chunk's centre (two_branch.py:226-228)
    int lo, lo2;                          // first frame of the first / last chunk
    const float* tubes;                   // [N, Tl, 5] or NULL (inference)
    const float* targets; int tstride;    // [N, 3, 6 + NC] fp32, tstride = 3 * (6 + NC); NULL: no losses
    float* prob; float* local_loc; float* first_loc; float* last_loc;      // [N,NC], [N,Tl,4], [N,T,4], [N,T,4]
    float* loss_cls; float* loss_loc; float* loss_nbr;                     // [N,NC], [1], [1]
    // backward
    const float* g_cls; const float* g_loc; const float* g_nbr;           // upstream gradients ([N,NC] | NULL, [1] | NULL, [1] | NULL)
    void* g_logits; void* g_reg;          // [N*Tl, NC], [N*Tl, 12] dense, activation dtype
};

template <typename T> __device__ __forceinline__ float ld(const void* p, size_t i) { return elem<T>::to_f32(((const T*)p)[i]); }
template <typename T> __device__ __forceinline__ void st(void* p, size_t i, float v) { ((T*)p)[i] = elem<T>::from_f32(v); }

// fixed-order block sum of one float per thread (256 threads): strided partials, then a tree in LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// encode_coef of one coordinate k (utils/tube_utils.py:139-157): gt box g[4], proposal a[4] (x1,y1,x2,y2), "+1" sizes
__device__ __forceinline__ float encode_k(const float* g, const float* a, int k) {
    const float gw = g[2] - g[0] + 1.0f, gh = g[3] - g[1] + 1.0f, w = a[2] - a[0] + 1.0f, h = a[3] - a[1] + 1.0f;
    switch (k) {
        case 0: return ((g[0] + 0.5f * gw) - (a[0] + 0.5f * w)) / w;
        case 1: return ((g[1] + 0.5f * gh) - (a[1] + 0.5f * h)) / h;
        case 2: return logf(gw / w);
        default: return logf(gh / h);
    }
}
__device__ __forceinline__ float smooth_l1(float d) { const float a = fabsf(d); return a < 1.0f ? 0.5f * d * d : a - 0.5f; }
__device__ __forceinline__ float smooth_l1_grad(float d) { return fabsf(d) < 1.0f ? d : (d > 0.f ? 1.0f : -1.0f); }

template <typename T>
__device__ __forceinline__ float mean_logit(const HeadParams& p, int n, int c) {
    float s = 0.f;
    for (int t = 0; t < p.Tl; ++t) s += ld<T>(p.logits, (size_t)(n * p.Tl + t) * p.lcs + c);
    return s / (float)p.Tl;
}
// the three regression predictions of tube n, coordinate k, and their targets / masks: j = 0 centre, 1 first, 2 last
template <typename T>
__device__ __forceinline__ void reg_terms(const HeadParams& p, int n, int k, float (&pred)[3], float (&tgt)[3], float (&msk)[3]) {
    const int fr[3] = {p.c_mid, p.c_first, p.c_last};
    const int tg[3] = {1, 0, 2};                                          // targets[:, 1] centre, [:, 0] first, [:, -1] last
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t row = (size_t)(n * p.Tl + fr[j]);
        float v = ld<T>(p.reg, row * p.rcs + k);
        if (j) v = v + ld<T>(p.reg, row * p.rcs + 4 * j + k);              // first: columns 4..7, last: 8..11 (two_branch.py:265-270)
        pred[j] = v;
        const float* tr = p.targets + (size_t)n * p.tstride + (size_t)tg[j] * (p.tstride / 3);
        tgt[j] = encode_k(tr, p.tubes + ((size_t)n * p.Tl + fr[j]) * 5 + 1, k);
        msk[j] = tr[5];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void head_outputs_kernel(HeadParams p) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const bool train = p.targets != nullptr;
    float pos = 0.f;
    if (train) {
        float m = 0.f;
        for (int n = tid; n < p.N; n += 256) m += p.targets[(size_t)n * p.tstride + (p.tstride / 3) + 4];
        pos = block_sum(m, red) > 0.f ? 1.f : 0.f;                          // `if mask.sum():` (two_branch.py:289)
    }
    // (inference launches several workgroups over the element-wise parts; training -- whose losses are block sums -- exactly one)
    const int gtid = blockIdx.x * 256 + tid, gstep = gridDim.x * 256;
    for (int i = gtid; i < p.N * p.NC; i += gstep) {
        const int n = i / p.NC, c = i % p.NC;
        const float x = mean_logit<T>(p, n, c);
        p.prob[i] = 1.0f / (1.0f + expf(-x));
        if (train) {
            const float* ct = p.targets + (size_t)n * p.tstride + (p.tstride / 3);
            const float t = ct[6 + c] * ct[4];
            // (a masked target drops the product instead of multiplying by 0: +inf under a 0 target is a loss of +inf, as torch's (1 - t) * x, not inf * 0 = NaN)
            p.loss_cls[i] = pos * (relu_nan(x) - (t != 0.f ? x * t : 0.f) + log1pf(expf(-fabsf(x))));
        }
    }
    if (p.reg) {
        for (int i = gtid; i < p.N * p.Tl * 4; i += gstep) {
            const int k = i & 3, row = i >> 2;
            p.local_loc[i] = ld<T>(p.reg, (size_t)row * p.rcs + k);
        }
        for (int i = gtid; i < p.N * p.T * 4; i += gstep) {
            const int k = i & 3, t = (i >> 2) % p.T, n = (i >> 2) / p.T;
            const size_t r1 = (size_t)(n * p.Tl + p.lo + t), r2 = (size_t)(n * p.Tl + p.lo2 + t);
            p.first_loc[i] = ld<T>(p.reg, r1 * p.rcs + k) + ld<T>(p.reg, r1 * p.rcs + 4 + k);
            p.last_loc[i] = ld<T>(p.reg, r2 * p.rcs + k) + ld<T>(p.reg, r2 * p.rcs + 8 + k);
        }
        if (train) {
            float sl = 0.f, sm = 0.f, snl = 0.f, snm = 0.f;
            for (int i = tid; i < p.N * 4; i += 256) {
                float pred[3], tgt[3], msk[3];
                reg_terms<T>(p, i >> 2, i & 3, pred, tgt, msk);
                sl += smooth_l1(pred[0] - tgt[0]) * msk[0]; sm += msk[0];
                snl += smooth_l1(pred[1] - tgt[1]) * msk[1] + smooth_l1(pred[2] - tgt[2]) * msk[2]; snm += msk[1] + msk[2];
            }
            const float L = block_sum(sl, red), M = block_sum(sm, red), NL = block_sum(snl, red), NM = block_sum(snm, red);
            if (tid == 0) {
                p.loss_loc[0] = M > 0.f ? L / M : 0.f;
                p.loss_nbr[0] = NM > 0.f ? NL / NM : 0.f;
            }
        }
    }
    if (!train && gtid < 3) {                                                // inference: three separate zero losses (two_branch.py:276-278)
        if (tid == 0) p.loss_cls[0] = 0.f;
        if (tid == 1) p.loss_loc[0] = 0.f;
        if (tid == 2) p.loss_nbr[0] = 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void head_outputs_bwd_kernel(HeadParams p) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float m = 0.f, sm = 0.f, snm = 0.f;
    for (int n = tid; n < p.N; n += 256) {
        const float* t3 = p.targets + (size_t)n * p.tstride;
        const int s = p.tstride / 3;
        m += t3[s + 4]; sm += 4.f * t3[s + 5]; snm += 4.f * (t3[5] + t3[2 * s + 5]);
    }
    const float pos = block_sum(m, red) > 0.f ? 1.f : 0.f;
    const float M = block_sum(sm, red), NM = block_sum(snm, red);
    const float gl = (p.g_loc && M > 0.f) ? p.g_loc[0] / M : 0.f;
    const float gn = (p.g_nbr && NM > 0.f) ? p.g_nbr[0] / NM : 0.f;
    // d loss_cls[n][c] / d logits[n][t][c] = (sigmoid(x) - t) * pos / Tl
    for (int i = tid; i < p.N * p.NC; i += 256) {
        const int n = i / p.NC, c = i % p.NC;
        float g = 0.f;
        if (p.g_cls) {
            const float x = mean_logit<T>(p, n, c);
            const float* ct = p.targets + (size_t)n * p.tstride + (p.tstride / 3);
            g = p.g_cls[i] * pos * (1.0f / (1.0f + expf(-x)) - ct[6 + c] * ct[4]) / (float)p.Tl;
        }
        for (int t = 0; t < p.Tl; ++t) st<T>(p.g_logits, (size_t)(n * p.Tl + t) * p.NC + c, g);
    }
    if (p.g_reg) {
        for (int i = tid; i < p.N * p.Tl * 12; i += 256) {
            const int j = i % 12, t = (i / 12) % p.Tl, n = i / (12 * p.Tl);
            const int k = j & 3, blk = j >> 2;                               // blk 0: local_reg, 1: neighbor_reg1 (first), 2: neighbor_reg2 (last)
            float v = 0.f;
            if (t == p.c_mid || t == p.c_first || t == p.c_last) {
                float pred[3], tgt[3], msk[3];
                reg_terms<T>(p, n, k, pred, tgt, msk);
                const float gc = gl * msk[0] * smooth_l1_grad(pred[0] - tgt[0]);
                const float gf = gn * msk[1] * smooth_l1_grad(pred[1] - tgt[1]);
                const float gla = gn * msk[2] * smooth_l1_grad(pred[2] - tgt[2]);
                if (blk == 0) v = (t == p.c_mid ? gc : 0.f) + (t == p.c_first ? gf : 0.f) + (t == p.c_last ? gla : 0.f);
                else if (blk == 1) v = t == p.c_first ? gf : 0.f;
                else v = t == p.c_last ? gla : 0.f;
            }
            st<T>(p.g_reg, (size_t)i, v);
        }
    }
}

// ---- dropout (models/two_branch.py:244-263: three call sites per head) ---------------------------------------------------------------
// A counter-based stream, so that a mask is a pure function of (seed, offset, element index): Philox4x32-10 (Random123), key = the
// seed's two halves, counter = (blk_lo, blk_hi, offset_lo, offset_hi) with blk = e >> 2, element e takes word e & 3 of its block.
// {seed, offset} live on the device; a one-thread kernel behind the pass bumps the offset, so a replayed graph draws a fresh mask on
// every replay (the pattern of step_sgd_flat_dev's counter).  include/step_amd.h has the definition in full; philox4x32_10 itself is in
// common.h (step_select_train in tube.hip draws from the same stream).
template <typename T> union vec16 { u32x4 q; T e[elem<T>::VEC]; };

// round_to_dtype(float(x) * scale), scale > 0.  For fp16 the compiler folds the widening, the multiply and the narrowing into one
// v_fma_mixlo_f16 with a +0 addend, and (-0) * scale + (+0) is +0: a kept -0 would lose its sign (seen on the MI355X; the interpreter
// build multiplies and converts separately).  The product is symmetric in the sign of x, so fp16 scales |x| and puts the sign bit back.
template <typename T> __device__ __forceinline__ T drop_scale(T x, float scale) { return elem<T>::from_f32(elem<T>::to_f32(x) * scale); }
template <> __device__ __forceinline__ f16_t drop_scale<f16_t>(f16_t x, float scale) {
    f16_t r;
    r.v = (unsigned short)(f32_to_f16_bits(fabsf(f16_bits_to_f32(x.v)) * scale) | (x.v & 0x8000u));
    return r;
}

constexpr int DROP_PER_LANE = 32;                        // elements per thread = one mask word's worth
constexpr int DROP_PER_WAVE = 64 * DROP_PER_LANE;
constexpr int DROP_PER_BLOCK = 4 * DROP_PER_WAVE;

// One wave covers 2048 consecutive elements in 32 / VEC load instructions of 16 bytes per lane, lanes contiguous within each
// instruction.  A mask word (32 elements) therefore spans NL = 32 / VEC neighbouring lanes of ONE instruction: every lane collects its
// VEC keep bits per instruction into `mine` (field j = instruction j), and a shuffle transpose inside each group of NL lanes hands lane q of
// the group the whole word of instruction q -- 64 words per wave, one store per lane, no atomics.  Elements past n keep bit 0 and are
// neither read nor written (partial vectors and misaligned tensors go element by element).
template <typename T>
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const T* x, T* y, uint32_t* mask, long long n, unsigned long long thr, float scale,
                                                          const unsigned long long* rng, int vec_ok) {
    constexpr int V = elem<T>::VEC, NL = DROP_PER_LANE / V;
    const int lane = threadIdx.x & 63;
    const long long wbase = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * DROP_PER_WAVE;
    if (wbase >= n) return;                                                  // (whole waves only: the shuffles below stay convergent)
    const unsigned long long seed = rng[0], off = rng[1];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), o0 = (unsigned)off, o1 = (unsigned)(off >> 32);
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const long long e0 = wbase + (long long)j * (64 * V) + lane * V;
        if (e0 >= n) continue;
        const bool full = vec_ok && e0 + V <= n;
        vec16<T> v, o;
        if (full) {
            v.q = *(const u32x4*)(x + e0);
        } else {
            for (int i = 0; i < V; ++i) v.e[i] = e0 + i < n ? x[e0 + i] : elem<T>::from_f32(0.f);
        }
        unsigned bits = 0;
#pragma unroll
        for (int b = 0; b < V / 4; ++b) {
            const unsigned long long blk = (unsigned long long)(e0 >> 2) + b;
            unsigned w[4];
            philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), o0, o1, k0, k1, w);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool keep = (unsigned long long)w[i] >= thr && e0 + 4 * b + i < n;
                o.e[4 * b + i] = keep ? drop_scale<T>(v.e[4 * b + i], scale) : elem<T>::from_f32(0.f);         // dropped: +0 by selection
                bits |= (keep ? 1u : 0u) << (4 * b + i);
            }
        }
        if (full) {
            *(u32x4*)(y + e0) = o.q;
        } else {
            for (int i = 0; i < V; ++i) if (e0 + i < n) y[e0 + i] = o.e[i];
        }
        mine |= bits << (V * j);
    }
    const int grp = lane / NL, q = lane % NL;
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const unsigned t = __shfl(mine, grp * NL + k);
        word |= ((t >> (V * q)) & ((1u << V) - 1u)) << (V * k);
    }
    const long long wi = (wbase >> 5) + q * (64 / NL) + grp;               // instruction q covers 64 * V elements = 64 / NL words
    if (wi < (n + 31) >> 5) mask[wi] = word;
}

// gx = bit ? round(float(gy) * scale) : +0 from the stored mask; the same element-to-lane map as the forward pass
template <typename T>
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const T* gy, T* gx, const uint32_t* mask, long long n, float scale, int vec_ok) {
    constexpr int V = elem<T>::VEC, NL = DROP_PER_LANE / V;
    const int lane = threadIdx.x & 63;
    const long long wbase = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * DROP_PER_WAVE;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const long long e0 = wbase + (long long)j * (64 * V) + lane * V;
        if (e0 >= n) continue;
        const bool full = vec_ok && e0 + V <= n;
        const unsigned bits = mask[e0 >> 5] >> (unsigned)(e0 & 31);
        vec16<T> v, o;
        if (full) {
            v.q = *(const u32x4*)(gy + e0);
        } else {
            for (int i = 0; i < V; ++i) v.e[i] = e0 + i < n ? gy[e0 + i] : elem<T>::from_f32(0.f);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) o.e[i] = ((bits >> i) & 1u) ? drop_scale<T>(v.e[i], scale) : elem<T>::from_f32(0.f);
        if (full) {
            *(u32x4*)(gx + e0) = o.q;
        } else {
            for (int i = 0; i < V; ++i) if (e0 + i < n) gx[e0 + i] = o.e[i];
        }
    }
}

__global__ __launch_bounds__(64) void rng_advance_kernel(unsigned long long* rng) {
    if (threadIdx.x == 0 && blockIdx.x == 0) rng[1] += 1ull;
}

__global__ __launch_bounds__(256) void rng_words_kernel(const unsigned long long* rng, unsigned long long first_blk, long long n_blk, uint32_t* out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_blk) return;
    const unsigned long long seed = rng[0], off = rng[1], blk = first_blk + (unsigned long long)t;
    unsigned w[4];
    philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), (unsigned)off, (unsigned)(off >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
    for (int i = 0; i < 4; ++i) out[4 * t + i] = w[i];
}

}  // namespace step

using namespace step;

extern "C" {

static int head_fill(HeadParams& p, int dtype, const void* logits, int lcs, const void* reg, int rcs, int N, int Tl, int T, int NC,
                     const float* tubes, const float* targets) {
    if (N < 0 || Tl <= 0 || T <= 0 || NC <= 0 || (Tl % T) != 0 || lcs < NC || (reg && rcs < 12)) return STEP_E_SHAPE;
    if (dtype != STEP_F32 && dtype != STEP_BF16 && dtype != STEP_F16) return STEP_E_DTYPE;
    if ((long long)N * Tl * (NC > 12 ? NC : 12) > 0x7fffffffLL) return STEP_E_UNSUPPORTED;
    const int chunks = Tl / T, half = T / 2;
    p.logits = logits; p.lcs = lcs; p.reg = reg; p.rcs = rcs;
    p.N = N; p.Tl = Tl; p.T = T; p.NC = NC;
    p.c_first = half; p.c_mid = (chunks / 2) * T + half; p.c_last = (chunks - 1) * T + half;      // chunk_idx[0], [chunks / 2], [-1]
    p.lo = 0; p.lo2 = (chunks - 1) * T;
    p.tubes = tubes; p.targets = targets; p.tstride = 3 * (6 + NC);
    return STEP_OK;
}

int step_head_outputs(int dtype, const void* logits, int logits_stride, const void* reg, int reg_stride, int N, int Tl, int T, int NC,
                      const float* tubes, const float* targets, float* prob, float* local_loc, float* first_loc, float* last_loc,
                      float* loss_cls, float* loss_loc, float* loss_nbr, step_stream_t stream) {
    HeadParams p = {};
    const int rc = head_fill(p, dtype, logits, logits_stride, reg, reg_stride, N, Tl, T, NC, tubes, targets);
    if (rc) return rc;
    if (!loss_cls || !loss_loc || !loss_nbr) return STEP_E_NULL;
    if (N > 0 && (!logits || !prob || (reg && (!local_loc || !first_loc || !last_loc)) || (targets && reg && !tubes))) return STEP_E_NULL;
    p.prob = prob; p.local_loc = local_loc; p.first_loc = first_loc; p.last_loc = last_loc;
    p.loss_cls = loss_cls; p.loss_loc = loss_loc; p.loss_nbr = loss_nbr;
    const long long work = (long long)N * (NC > Tl * 4 ? NC : Tl * 4);
    const dim3 grid(targets ? 1u : (unsigned)(work <= 256 ? 1 : (work + 255) / 256 > 64 ? 64 : (work + 255) / 256));
    switch (dtype) {
        case STEP_F32: STEP_LAUNCH((head_outputs_kernel<float>), grid, dim3(256), stream, p); break;
        case STEP_BF16: STEP_LAUNCH((head_outputs_kernel<bf16_t>), grid, dim3(256), stream, p); break;
        default: STEP_LAUNCH((head_outputs_kernel<f16_t>), grid, dim3(256), stream, p); break;
    }
    return STEP_LAUNCH_CHECK();
}

int step_head_outputs_backward(int dtype, const void* logits, int logits_stride, const void* reg, int reg_stride, int N, int Tl, int T, int NC,
                               const float* tubes, const float* targets, const float* g_loss_cls, const float* g_loss_loc,
                               const float* g_loss_nbr, void* g_logits, void* g_reg, step_stream_t stream) {
    HeadParams p = {};
    const int rc = head_fill(p, dtype, logits, logits_stride, reg, reg_stride, N, Tl, T, NC, tubes, targets);
    if (rc) return rc;
    if (N == 0) return STEP_OK;
    if (!logits || !targets || !g_logits || (reg && (!tubes || !g_reg))) return STEP_E_NULL;
    p.g_cls = g_loss_cls; p.g_loc = g_loss_loc; p.g_nbr = g_loss_nbr; p.g_logits = g_logits; p.g_reg = reg ? g_reg : nullptr;
    switch (dtype) {
        case STEP_F32: STEP_LAUNCH((head_outputs_bwd_kernel<float>), dim3(1), dim3(256), stream, p); break;
        case STEP_BF16: STEP_LAUNCH((head_outputs_bwd_kernel<bf16_t>), dim3(1), dim3(256), stream, p); break;
        default: STEP_LAUNCH((head_outputs_bwd_kernel<f16_t>), dim3(1), dim3(256), stream, p); break;
    }
    return STEP_LAUNCH_CHECK();
}

// keep threshold and scale of a drop probability: keep iff (uint64)word >= floor(p * 2^32), scale = 1 / (1 - p) taken in double
static int dropout_consts(int dtype, long long n, double p, unsigned long long& thr, float& scale, long long& blocks) {
    if (dtype != STEP_F32 && dtype != STEP_BF16 && dtype != STEP_F16) return STEP_E_DTYPE;
    if (n < 0 || !(p >= 0.0 && p <= 1.0)) return STEP_E_SHAPE;
    blocks = (n + DROP_PER_BLOCK - 1) / DROP_PER_BLOCK;
    if (blocks > 0x7fffffffLL) return STEP_E_UNSUPPORTED;
    thr = (unsigned long long)std::floor(p * 4294967296.0);
    scale = p == 1.0 ? 0.f : (float)(1.0 / (1.0 - p));
    return STEP_OK;
}

int step_dropout_forward(int dtype, const void* x, void* y, uint32_t* mask, long long n, double p, unsigned long long* rng_state,
                         step_stream_t stream) {
    unsigned long long thr; float scale; long long blocks;
    const int rc = dropout_consts(dtype, n, p, thr, scale, blocks);
    if (rc) return rc;
    if (!rng_state || (n > 0 && (!x || !y || !mask))) return STEP_E_NULL;
    const int es = dtype == STEP_F32 ? 4 : 2;
    if ((((uintptr_t)x) | ((uintptr_t)y)) & (es - 1) || ((uintptr_t)mask & 3) || ((uintptr_t)rng_state & 7)) return STEP_E_ALIGN;
    const int vec_ok = ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0;
    if (n > 0) {
        const dim3 grid((unsigned)blocks);
        switch (dtype) {
            case STEP_F32: STEP_LAUNCH((dropout_fwd_kernel<float>), grid, dim3(256), stream, (const float*)x, (float*)y, mask, n, thr, scale, (const unsigned long long*)rng_state, vec_ok); break;
            case STEP_BF16: STEP_LAUNCH((dropout_fwd_kernel<bf16_t>), grid, dim3(256), stream, (const bf16_t*)x, (bf16_t*)y, mask, n, thr, scale, (const unsigned long long*)rng_state, vec_ok); break;
            default: STEP_LAUNCH((dropout_fwd_kernel<f16_t>), grid, dim3(256), stream, (const f16_t*)x, (f16_t*)y, mask, n, thr, scale, (const unsigned long long*)rng_state, vec_ok); break;
        }
    }
    STEP_LAUNCH(rng_advance_kernel, dim3(1), dim3(64), stream, rng_state);     // (also for n == 0: the call counts)
    return STEP_LAUNCH_CHECK();
}

int step_dropout_backward(int dtype, const void* gy, void* gx, const uint32_t* mask, long long n, double p, step_stream_t stream) {
    unsigned long long thr; float scale; long long blocks;
    const int rc = dropout_consts(dtype, n, p, thr, scale, blocks);
    if (rc) return rc;
    if (n == 0) return STEP_OK;
    if (!gy || !gx || !mask) return STEP_E_NULL;
    const int es = dtype == STEP_F32 ? 4 : 2;
    if ((((uintptr_t)gy) | ((uintptr_t)gx)) & (es - 1) || ((uintptr_t)mask & 3)) return STEP_E_ALIGN;
    const int vec_ok = ((((uintptr_t)gy) | ((uintptr_t)gx)) & 15) == 0;
    const dim3 grid((unsigned)blocks);
    switch (dtype) {
        case STEP_F32: STEP_LAUNCH((dropout_bwd_kernel<float>), grid, dim3(256), stream, (const float*)gy, (float*)gx, mask, n, scale, vec_ok); break;
        case STEP_BF16: STEP_LAUNCH((dropout_bwd_kernel<bf16_t>), grid, dim3(256), stream, (const bf16_t*)gy, (bf16_t*)gx, mask, n, scale, vec_ok); break;
        default: STEP_LAUNCH((dropout_bwd_kernel<f16_t>), grid, dim3(256), stream, (const f16_t*)gy, (f16_t*)gx, mask, n, scale, vec_ok); break;
    }
    return STEP_LAUNCH_CHECK();
}

int step_rng_words(const unsigned long long* rng_state, unsigned long long first_blk, long long n_blk, uint32_t* out, step_stream_t stream) {
    if (n_blk < 0) return STEP_E_SHAPE;
    if (n_blk == 0) return STEP_OK;
    if (!rng_state || !out) return STEP_E_NULL;
    const long long blocks = (n_blk + 255) / 256;
    if (blocks > 0x7fffffffLL) return STEP_E_UNSUPPORTED;
    STEP_LAUNCH(rng_words_kernel, dim3((unsigned)blocks), dim3(256), stream, rng_state, first_blk, n_blk, out);
    return STEP_LAUNCH_CHECK();
}

}  // extern "C"
