// step_amd/csrc/optim.hip -- fused multi-tensor Adam and SGD-with-momentum over flat fp32 parameter arenas.
//
// Replaces optimizer.step() of torch.optim.Adam(params, lr=args.det_lr) (reference train.py:126,348) over the 159+
// single-tensor parameter groups utils/solver.py:12-93 builds (per-group lr and weight_decay): the reference runs
// a handful of element-wise kernels per group; here all parameters, gradients and both moments live in four flat
// arenas and ONE launch updates them.  Pure HBM streaming: 16 B read + 12 B written per element (+4 B when the
// gradient is cleared in the same pass), no reuse -> bound by HBM bandwidth; 16-byte vectors, grid-stride.
//
// Arithmetic follows torch/optim/adam.py::_single_tensor_adam (amsgrad=False, maximize=False):
//   g  = grad * grad_scale (+ weight_decay * p)
//   m += (g - m) * (1 - beta1)                 (Tensor.lerp_)
//   v  = v * beta2 + (1 - beta2) * g * g
//   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// Also here, beside the optimizers they feed: the bf16 wire of the data-parallel gradient exchange (grad_pack16 / grad_unpack16), the
// gradient-norm clip in front of them (grad_norm / grad_clip) and the learning-rate schedules that write their seg_lr table (lr_schedule).
#include "common.h"
#include <cmath>
#include <cstdlib>

namespace step {

constexpr int ADAM_MAX_SEG = 4096;      // 32 KiB of LDS for the segment table

template <int MAXSEG>
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long long nvec,
                                                        const long long* __restrict__ seg_end, const float* __restrict__ seg_lr,
                                                        const float* __restrict__ seg_wd, int n_seg, float beta2, float omb1,
                                                        float omb2, float eps, float bc1, float bc2_sqrt, float gscale,
                                                        int zero_grad, const float* __restrict__ bc_dev, const float* __restrict__ amp) {
    __shared__ long long s_end[MAXSEG];                    // 4 KiB for the usual few hundred tensors: LDS does not limit occupancy
    if (bc_dev) { bc1 = bc_dev[0]; bc2_sqrt = bc_dev[1]; } // step counter on the device (adam_bias_kernel): graph replays advance it
    // dynamic loss scaling (step_adam_flat_amp): amp = {scale, growth_tracker, found_inf, -}.  The gradients carry the factor `scale`;
    // a step whose gradients held an inf / nan is SKIPPED (apex amp O1's patched optimizer.step, torch.amp.GradScaler.step) -- no
    // moment decay, no parameter change; the gradient arena is still cleared when the caller asked for it.
    bool skip = false;
    if (amp) { skip = amp[2] != 0.f; gscale = gscale * (1.f / amp[0]); }
    for (int i = threadIdx.x; i < n_seg; i += blockDim.x) s_end[i] = seg_end[i];
    __syncthreads();
    for (long long vec = (long long)blockIdx.x * blockDim.x + threadIdx.x; vec < nvec; vec += (long long)blockDim.x * gridDim.x) {
        const long long e = vec * 4;
        int lo = 0, hi = n_seg - 1;                       // first segment whose end lies beyond e
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] > e) hi = mid; else lo = mid + 1;
        }
        if (skip) {
            if (zero_grad) *(f32x4*)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        const float lr = seg_lr[lo], wd = seg_wd[lo];
        const float step_size = lr / bc1;
        f32x4 P = *(const f32x4*)(p + e), G = *(const f32x4*)(g + e), M = *(const f32x4*)(m + e), V = *(const f32x4*)(v + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gj = G[j] * gscale;
            if (wd != 0.f) gj = gj + wd * P[j];
            const float mj = M[j] + (gj - M[j]) * omb1;
            const float vj = V[j] * beta2 + omb2 * gj * gj;
            const float denom = sqrtf(vj) / bc2_sqrt + eps;
            P[j] = P[j] - step_size * (mj / denom);
            M[j] = mj;
            V[j] = vj;
        }
        *(f32x4*)(p + e) = P;
        *(f32x4*)(m + e) = M;
        *(f32x4*)(v + e) = V;
        if (zero_grad) *(f32x4*)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// the step counter of a CAPTURED optimizer step lives on the device: a replayed graph cannot receive a new host scalar.  One
// thread advances it and leaves the two bias corrections (double precision, as the host path) for adam_flat_kernel.
__global__ void adam_bias_kernel(long long* step, float* bc, double beta1, double beta2, const float* amp) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (amp && amp[2] != 0.f) return;                  // skipped step (overflowed gradients): the step count does not advance
        const long long t = *step + 1;
        *step = t;
        bc[0] = (float)(1.0 - pow(beta1, (double)t));
        bc[1] = (float)sqrt(1.0 - pow(beta2, (double)t));
    }
}

// ---- dynamic loss scaling (mixed-precision training: train.py:136-139 `amp.initialize(opt_level="O1")`, :342-345 `amp.scale_loss`) ----
// amp_state = {scale, growth_tracker, found_inf, unused}: the state of apex's DynamicLossScaler / torch.amp.GradScaler, on the device so
// that a captured training step needs no host decision.  grad_scan raises found_inf when any gradient is inf / nan (the overflow check
// apex runs while unscaling); loss_scale_update is GradScaler.update(): overflow -> scale *= backoff, tracker = 0; else tracker += 1 and
// at growth_interval clean steps scale *= growth, tracker = 0; found_inf is cleared for the next step.
__global__ __launch_bounds__(256) void grad_scan_kernel(const float* __restrict__ g, long long nvec, float* __restrict__ amp) {
    bool bad = false;
    for (long long vec = (long long)blockIdx.x * blockDim.x + threadIdx.x; vec < nvec; vec += (long long)blockDim.x * gridDim.x) {
        const u32x4 v = *(const u32x4*)(g + vec * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) bad |= (v[j] & 0x7f800000u) == 0x7f800000u;     // exponent all ones: inf or nan
    }
    if (bad) amp[2] = 1.f;                                  // (every writer stores the same value)
}

__global__ void loss_scale_update_kernel(float* amp, float growth, float backoff, int interval) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (amp[2] != 0.f) { amp[0] = amp[0] * backoff; amp[1] = 0.f; }
        else {
            const float t = amp[1] + 1.f;
            if (t >= (float)interval) { amp[0] = amp[0] * growth; amp[1] = 0.f; }
            else amp[1] = t;
        }
        amp[2] = 0.f;
    }
}

// ---- SGD with momentum (the reference's DEFAULT optimizer: config.py:51 `--optimizer sgd`, train.py:123-124) ----------------------
// optim.SGD(params, lr=args.det_lr, momentum=args.momentum, weight_decay=args.weight_decay) over the same single-tensor groups, on
// THREE arenas (parameters, gradients, one momentum buffer): 12 B read + 8 B written per element (+4 B for the fused gradient clear),
// against Adam's 16 + 12.  Arithmetic follows torch/optim/sgd.py::_single_tensor_sgd (maximize=False), in its order:
//   g   = grad * grad_scale (+ weight_decay * p)
//   buf = g                                     on the FIRST step (torch clones the gradient: no dampening)
//   buf = momentum * buf + (1 - dampening) * g  afterwards
//   g   = g + momentum * buf  (nesterov)   |   g = buf
//   p  -= lr * g
// "first step" is a host scalar (step_sgd_flat: step == 1) or the OLD value of the device counter (step_sgd_flat_dev / _amp: *step_dev
// == 0), read once per thread ahead of the loop; sgd_count_kernel advances the counter BEHIND this pass on the same stream, so no
// thread of this launch reads a value another thread of it writes.  MOM = false (momentum == 0): no buffer is read or written.
template <int MAXSEG, bool MOM>
__global__ __launch_bounds__(256) void sgd_flat_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, long long nvec,
                                                       const long long* __restrict__ seg_end, const float* __restrict__ seg_lr,
                                                       const float* __restrict__ seg_wd, int n_seg, float mu, float omd, int nesterov,
                                                       int first, float gscale, int zero_grad, const long long* __restrict__ step_dev,
                                                       const float* __restrict__ amp) {
    __shared__ long long s_end[MAXSEG];
    if (step_dev) first = *step_dev == 0;                  // no clean step yet (a skipped step does not count): this one initialises the buffer
    bool skip = false;                                     // dynamic loss scaling: as adam_flat_kernel
    if (amp) { skip = amp[2] != 0.f; gscale = gscale * (1.f / amp[0]); }
    for (int i = threadIdx.x; i < n_seg; i += blockDim.x) s_end[i] = seg_end[i];
    __syncthreads();
    for (long long vec = (long long)blockIdx.x * blockDim.x + threadIdx.x; vec < nvec; vec += (long long)blockDim.x * gridDim.x) {
        const long long e = vec * 4;
        if (skip) {
            if (zero_grad) *(f32x4*)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        int lo = 0, hi = n_seg - 1;                       // first segment whose end lies beyond e
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] > e) hi = mid; else lo = mid + 1;
        }
        const float lr = seg_lr[lo], wd = seg_wd[lo];
        f32x4 P = *(const f32x4*)(p + e), G = *(const f32x4*)(g + e), B = f32x4{0.f, 0.f, 0.f, 0.f};
        if (MOM && !first) B = *(const f32x4*)(buf + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gj = G[j] * gscale;
            if (wd != 0.f) gj = gj + wd * P[j];
            if (MOM) {
                const float bj = first ? gj : mu * B[j] + omd * gj;
                B[j] = bj;
                gj = nesterov ? gj + mu * bj : bj;
            }
            P[j] = P[j] - lr * gj;
        }
        *(f32x4*)(p + e) = P;
        if (MOM) *(f32x4*)(buf + e) = B;
        if (zero_grad) *(f32x4*)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// the tail of a device-counted SGD step: one thread advances the counter once the main pass has read it (stream order).  A step
// skipped for overflow does not count, so the first CLEAN step is still the one that finds the counter at 0 and sets buf = g
// (torch.amp.GradScaler + SGD: a skipped step() leaves `momentum_buffer` absent).
__global__ void sgd_count_kernel(long long* step, const float* amp) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (amp && amp[2] != 0.f) return;
        *step = *step + 1;
    }
}

// ---- 16-bit gradient wire with error feedback (step_grad_pack16 / step_grad_unpack16; the data-parallel exchange of step_amd.dist) ----
// pack:   v = fma(grad, pre_scale, residual), wire = bf16(v) (round to nearest even), residual = v - float(wire) -- EXACT in fp32: |v -
//         float(wire)| <= half a bf16 ulp of v and a multiple of v's fp32 ulp, so it fits the 24-bit significand -- or 0 where the wire
//         value is inf / NaN (the overflow must travel, it must not stay in the residual).  14 B per element with a residual, 6 without.
// unpack: grad = float(wire), exact.  6 B per element.
// Pure HBM streaming like the optimizer passes: 256-thread workgroups, grid-stride, 8 elements per lane and iteration (16-byte vectors
// of all three tensors); VEC = false walks element by element (a view that does not start on a 16-byte line).  The conversion is the
// project's f32_to_bf16_bits, one v_cvt_pk_bf16_f32 per pair on the device.
__device__ __forceinline__ unsigned short pack16_one(float g, float r, float s, float& r_new) {
    const float v = fmaf(g, s, r);                         // ONE rounding, on the device and on the interpreter (-ffp-contract=off)
    const unsigned short w = f32_to_bf16_bits(v);
    r_new = (w & 0x7f80u) != 0x7f80u ? v - bf16_bits_to_f32(w) : 0.f;
    return w;
}

template <bool RES, bool VEC>
__global__ __launch_bounds__(256) void grad_pack16_kernel(const float* __restrict__ grad, float* __restrict__ residual,
                                                          unsigned short* __restrict__ wire, long long n, float pre_scale) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)blockDim.x * gridDim.x;
    long long done = 0;                                    // elements the vector body covers; the rest is the scalar tail
    if (VEC) {
        const long long nvec = n >> 3;
        done = nvec << 3;
        for (long long vec = gid; vec < nvec; vec += stride) {
            const long long e = vec * 8;
            const f32x4 g0 = *(const f32x4*)(grad + e), g1 = *(const f32x4*)(grad + e + 4);
            f32x4 r0 = f32x4{0.f, 0.f, 0.f, 0.f}, r1 = r0;
            if (RES) { r0 = *(const f32x4*)(residual + e); r1 = *(const f32x4*)(residual + e + 4); }
            u16x8 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a, b;
                w[j] = pack16_one(g0[j], r0[j], pre_scale, a);
                w[j + 4] = pack16_one(g1[j], r1[j], pre_scale, b);
                r0[j] = a; r1[j] = b;
            }
            *(u16x8*)(wire + e) = w;
            if (RES) { *(f32x4*)(residual + e) = r0; *(f32x4*)(residual + e + 4) = r1; }
        }
    }
    for (long long e = done + gid; e < n; e += stride) {
        float r = 0.f;
        wire[e] = pack16_one(grad[e], RES ? residual[e] : 0.f, pre_scale, r);
        if (RES) residual[e] = r;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void grad_unpack16_kernel(const unsigned short* __restrict__ wire, float* __restrict__ grad, long long n) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)blockDim.x * gridDim.x;
    long long done = 0;
    if (VEC) {
        const long long nvec = n >> 3;
        done = nvec << 3;
        for (long long vec = gid; vec < nvec; vec += stride) {
            const long long e = vec * 8;
            const u16x8 w = *(const u16x8*)(wire + e);
            *(f32x4*)(grad + e) = f32x4{bf16_bits_to_f32(w[0]), bf16_bits_to_f32(w[1]), bf16_bits_to_f32(w[2]), bf16_bits_to_f32(w[3])};
            *(f32x4*)(grad + e + 4) = f32x4{bf16_bits_to_f32(w[4]), bf16_bits_to_f32(w[5]), bf16_bits_to_f32(w[6]), bf16_bits_to_f32(w[7])};
        }
    }
    for (long long e = done + gid; e < n; e += stride) grad[e] = bf16_bits_to_f32(wire[e]);
}

// ---- gradient-norm clipping (step_grad_norm_flat / step_grad_clip_flat: torch.nn.utils.clip_grad_norm_ over the gradient arena) -----
// One streaming read of the arena (4 B per element, 16-byte vectors) + one single-workgroup finishing launch; the in-place multiply
// (8 B per element) only moves data on a step that is clipped.  Sums of squares are fp64 -- (double)g * (double)g is exact, so a
// contracted multiply-add and a separate one give the same bits, on the device and on the interpreter -- and their ORDER is fixed (the
// contract is spelled out in include/step_amd.h): chunks of GN_CHUNK elements at fixed positions, whichever workgroup of the grid-stride
// loop gets them; within a chunk a lane's vectors in ascending order, an xor butterfly across the wavefront (every lane ends with the same
// bits: each stage adds the same two numbers on both sides), the four wavefronts in index order.  No atomics.
constexpr int GN_CHUNK = STEP_GRAD_NORM_CHUNK;           // elements per chunk: 8 vectors per lane
constexpr int GN_VPL = GN_CHUNK / 4 / 256;               // vectors per lane and chunk
constexpr int GN_FIN_THREADS = 1024;                     // the finishing workgroup: 16 wavefronts ...
constexpr int GN_FIN_SEGS = 4;                           // ... each summing this many segments at a time ...
constexpr int GN_FIN_BATCH = 8;                          // ... from batches of this many loads per lane

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// first segment whose end lies beyond element e (the search of the optimizer kernels); n_seg - 1 where there is none
__device__ __forceinline__ int seg_of(const long long* s_end, int n_seg, long long e) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_end[mid] > e) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <int MAXSEG>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long long n, const long long* __restrict__ seg_end,
                                                                int n_seg, double* __restrict__ ws) {
    __shared__ long long s_end[MAXSEG];
    __shared__ double s_wave[2][4];
    int slot = 0;
    for (int i = threadIdx.x; i < n_seg; i += blockDim.x) s_end[i] = seg_end[i];
    __syncthreads();
    if (s_end[n_seg - 1] != n) return;                     // a table that does not describe this arena: nothing is written (uniform)
    const long long nchunk = (n + GN_CHUNK - 1) / GN_CHUNK, nvec = n >> 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const long long c0 = c * GN_CHUNK, c1 = c0 + GN_CHUNK < n ? c0 + GN_CHUNK : n;
        f32x4 v[GN_VPL];
#pragma unroll
        for (int j = 0; j < GN_VPL; ++j) {
            const long long vec = (c0 >> 2) + j * 256 + threadIdx.x;
            v[j] = vec < nvec ? *(const f32x4*)(g + vec * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int sa = seg_of(s_end, n_seg, c0), sb = seg_of(s_end, n_seg, c1 - 1);
        for (int s = sa; s <= sb; ++s) {                   // usually one turn: the chunk lies inside one tensor
            const long long lo = s > 0 ? s_end[s - 1] : 0, hi = s_end[s];
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < GN_VPL; ++j) {
                const long long e = c0 + 4LL * (j * 256 + threadIdx.x);
                if (sa == sb || (e >= lo && e < hi)) {     // (segment ends are multiples of 4: a vector never straddles two)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc += (double)v[j][k] * (double)v[j][k];
                }
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) s_wave[slot][wave] = acc;
            __syncthreads();                               // (two slots in turn: the barrier of the NEXT reduction orders this read before the slot's reuse)
            if (threadIdx.x == 0) ws[c + s] = ((s_wave[slot][0] + s_wave[slot][1]) + s_wave[slot][2]) + s_wave[slot][3];
            slot ^= 1;
        }
    }
}

__global__ __launch_bounds__(GN_FIN_THREADS) void grad_norm_finish_kernel(long long n, const long long* __restrict__ seg_end, int n_seg,
                                                                          const double* __restrict__ ws, float gscale,
                                                                          const float* __restrict__ amp, float max_norm,
                                                                          float* __restrict__ seg_norm, float* __restrict__ stats) {
    __shared__ double s_seg[ADAM_MAX_SEG];
    if (seg_end[n_seg - 1] != n) return;                   // as the streaming pass: refused on the device, nothing written
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const double mul = fabs((double)gscale), scale = amp ? (double)amp[0] : 1.0;
    // a wavefront sums GN_FIN_SEGS segments at a time: their loads are in flight together and their butterflies interleave.  Lane l adds
    // its segment's parts l, l + 64, ... in chunk order; a batch is loaded first and then added in that order, missing parts as + 0.0 (the
    // sums are >= 0: adding zero changes no bit)
    for (int s0 = wave * GN_FIN_SEGS; s0 < n_seg; s0 += nwave * GN_FIN_SEGS) {
        double acc[GN_FIN_SEGS];
        long long nxt[GN_FIN_SEGS], last[GN_FIN_SEGS];
#pragma unroll
        for (int q = 0; q < GN_FIN_SEGS; ++q) {
            const int s = s0 + q;
            long long c = lane, cb = -1;
            if (s < n_seg) {
                long long lo = s > 0 ? seg_end[s - 1] : 0, hi = seg_end[s];
                if (lo < 0) lo = 0;                        // (a table that is not ascending within [0, n] gives wrong sums, never a read outside
                if (hi > n) hi = n;                        //  the workspace)
                if (hi > lo) { c = lo / GN_CHUNK + lane; cb = (hi - 1) / GN_CHUNK; }
            }
            double v[GN_FIN_BATCH];
#pragma unroll
            for (int j = 0; j < GN_FIN_BATCH; ++j) v[j] = c + 64 * j <= cb ? ws[c + 64 * j + s] : 0.0;
            acc[q] = 0.0;
#pragma unroll
            for (int j = 0; j < GN_FIN_BATCH; ++j) acc[q] += v[j];
            nxt[q] = c + 64 * GN_FIN_BATCH;
            last[q] = cb;
        }
#pragma unroll
        for (int q = 0; q < GN_FIN_SEGS; ++q) {            // only a tensor beyond 64 x GN_FIN_BATCH chunks (4 M elements) comes here
            const int s = s0 + q;
            for (long long c = nxt[q]; c <= last[q]; c += 64 * GN_FIN_BATCH) {
                double v[GN_FIN_BATCH];
#pragma unroll
                for (int j = 0; j < GN_FIN_BATCH; ++j) v[j] = c + 64 * j <= last[q] ? ws[c + 64 * j + s] : 0.0;
#pragma unroll
                for (int j = 0; j < GN_FIN_BATCH; ++j) acc[q] += v[j];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
            for (int q = 0; q < GN_FIN_SEGS; ++q) acc[q] += __shfl_xor(acc[q], m);
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < GN_FIN_SEGS; ++q) {
                const int s = s0 + q;
                if (s < n_seg) {
                    s_seg[s] = acc[q];
                    if (seg_norm) seg_norm[s] = (float)(sqrt(acc[q]) * mul / scale);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < n_seg; ++s) tot += s_seg[s];
        const float norm = (float)(sqrt(tot) * mul / scale);
        const bool finite = (__builtin_bit_cast(unsigned int, norm) & 0x7f800000u) != 0x7f800000u;
        float coef = 1.f;
        if (finite) {
            coef = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
            if (!(coef < 1.f)) coef = 1.f;
        }
        stats[0] = norm; stats[1] = coef; stats[2] = finite ? 0.f : 1.f; stats[3] = 0.f;
    }
}

__global__ __launch_bounds__(256) void grad_clip_kernel(float* __restrict__ g, long long nvec, const float* __restrict__ stats) {
    const float coef = stats[1];
    if (coef == 1.f) return;                               // not clipped: x * 1.0f == x bit for bit, so nothing is read or written
    for (long long vec = (long long)blockIdx.x * blockDim.x + threadIdx.x; vec < nvec; vec += (long long)blockDim.x * gridDim.x) {
        f32x4 G = *(const f32x4*)(g + vec * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) G[j] = G[j] * coef;
        *(f32x4*)(g + vec * 4) = G;
    }
}

// ---- the reference's learning-rate schedules on the device (step_lr_schedule; utils/solver.py:96-172) --------------------------------
// One workgroup: every thread reads the counter, a barrier, thread 0 writes it back incremented; then one thread per segment evaluates
// get_lr() for the new last_epoch in fp64 -- the operations and their order are Python's -- and rounds once to fp32.
constexpr int LR_MAX_MS = STEP_LR_MAX_MILESTONES;

__device__ __forceinline__ int bisect_right_ll(const long long* a, int n, long long x) {
    int k = 0;
    while (k < n && a[k] <= x) ++k;
    return k;
}

__global__ __launch_bounds__(256) void lr_schedule_kernel(int kind, long long* iter, const double* __restrict__ base_lr, float* __restrict__ seg_lr,
                                                          int n_seg, const long long* __restrict__ milestones, int n_ms, long long warmup_iters,
                                                          double warmup_factor, double p0, double p1) {
    __shared__ long long s_ms[LR_MAX_MS];
    const long long t = *iter + 1;
    for (int i = threadIdx.x; i < n_ms; i += blockDim.x) s_ms[i] = milestones[i];
    __syncthreads();
    if (threadIdx.x == 0) *iter = t;
    double factor = 0.0, floor_ratio = 0.0;                // lr = base * floor_ratio + (base * factor - base * floor_ratio) * shape, or base * factor
    double shape = 0.0;
    const bool warm = t < warmup_iters;
    if (warm) {
        const double alpha = (double)t / (double)warmup_iters;
        factor = warmup_factor * (1.0 - alpha) + alpha;
    } else if (kind == STEP_LR_COSINE) {
        int cycle = bisect_right_ll(s_ms, n_ms, t);
        if (cycle > n_ms - 1) cycle = n_ms - 1;
        if (cycle < 1) cycle = 1;                          // (a table whose first entry is not warmup_iters: stay inside it)
        double fraction = (double)(t - s_ms[cycle - 1]) / (double)(s_ms[cycle] - s_ms[cycle - 1]);
        if (!(fraction < 1.0)) fraction = 1.0;
        factor = pow(p1, (double)(cycle - 1));
        floor_ratio = p0;
        shape = 1.0 + cos(3.141592653589793 * fraction);
    } else {
        factor = pow(p0, (double)bisect_right_ll(s_ms, n_ms, t));
    }
    for (int s = threadIdx.x; s < n_seg; s += blockDim.x) {
        const double base = base_lr[s];
        double lr;
        if (warm || kind != STEP_LR_COSINE) lr = base * factor;
        else lr = base * floor_ratio + (base * factor - base * floor_ratio) * shape / 2.0;
        seg_lr[s] = (float)lr;
    }
}

// ---- activation gradient of the fused conv unit ---------------------------------------------------------------------
// backward of  y = relu(conv * scale[c] + shift[c])  up to the conv:  g = gy * (y > 0) * scale[c], written once as fp32
// (operand of the weight-gradient kernel) and / or once in the activation dtype (operand of the data-gradient conv).
// One read of y and gy instead of the cast / compare / multiply / multiply / cast chain of element-wise passes.
typedef unsigned short u16x4_t __attribute__((ext_vector_type(4)));
template <typename T> struct Vec4;
template <> struct Vec4<float> {
    __device__ static __forceinline__ f32x4 load(const float* p) { return *(const f32x4*)p; }
    __device__ static __forceinline__ void store(float* p, const f32x4& v) { *(f32x4*)p = v; }
};
template <typename T> struct Vec4 {
    __device__ static __forceinline__ f32x4 load(const T* p) {
        const u16x4_t r = *(const u16x4_t*)p;
        return f32x4{elem<T>::from_bits16(r[0]), elem<T>::from_bits16(r[1]), elem<T>::from_bits16(r[2]), elem<T>::from_bits16(r[3])};
    }
    __device__ static __forceinline__ void store(T* p, const f32x4& v) {
        *(u16x4_t*)p = u16x4_t{elem<T>::bits16(v[0]), elem<T>::bits16(v[1]), elem<T>::bits16(v[2]), elem<T>::bits16(v[3])};
    }
};

template <typename TY, typename TG>
__global__ __launch_bounds__(256) void act_grad_kernel(const TY* __restrict__ y, const TG* __restrict__ gy, const float* __restrict__ scale,
                                                       long long nvec, int C, int y_cs, int gy_cs, int relu, float* __restrict__ g32,
                                                       TY* __restrict__ gt) {
    const int cv = C >> 2;                                                   // C % 4 == 0: a vector never straddles two pixels
    for (long long vec = (long long)blockIdx.x * blockDim.x + threadIdx.x; vec < nvec; vec += (long long)blockDim.x * gridDim.x) {
        const long long m = vec / cv;                                        // pixel; y / gy may be channel slices of wider buffers
        const int c = (int)(vec - m * cv) << 2;
        const long long e = vec * 4;                                         // the outputs are dense [M, C]
        f32x4 g = Vec4<TG>::load(gy + m * gy_cs + c);
        if (scale) {
            const f32x4 s = *(const f32x4*)(scale + c);
            g = f32x4{g[0] * s[0], g[1] * s[1], g[2] * s[2], g[3] * s[3]};
        }
        if (relu) {
            const f32x4 yv = Vec4<TY>::load(y + m * y_cs + c);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(yv[j] > 0.f)) g[j] = 0.f;
        }
        if (g32) *(f32x4*)(g32 + e) = g;
        if (gt) Vec4<TY>::store(gt + e, g);
    }
}

// 16-bit activations, C % 8 == 0: a 16-byte vector per lane and iteration, the (pixel, channel) pair of the grid-stride walk carried
// incrementally (the 4-wide form above pays a 64-bit division per 8 bytes: measured 1.6 TB/s of operand traffic over the 72 calls of
// a training step).  Same arithmetic per element -- fp32 product, mask, one rounding -- so the two forms agree bit for bit.
template <typename TY, typename TG>
__global__ __launch_bounds__(256) void act_grad8_kernel(const TY* __restrict__ y, const TG* __restrict__ gy, const float* __restrict__ scale,
                                                        long long nvec, int C, int y_cs, int gy_cs, int relu, float* __restrict__ g32,
                                                        TY* __restrict__ gt) {
    static_assert(sizeof(TY) == 2, "16-bit activations");
    const int cv = C >> 3;
    const long long stride = (long long)blockDim.x * gridDim.x;
    long long vec = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec >= nvec) return;
    long long m = vec / cv;
    int c = (int)(vec - m * cv);
    const long long dm = stride / cv;
    const int dc = (int)(stride - dm * cv);
    for (; vec < nvec; vec += stride) {
        float g[8];
        const TG* gp = gy + m * gy_cs + c * 8;
        if constexpr (sizeof(TG) == 4) {
            const f32x4 a = *(const f32x4*)gp, b = *(const f32x4*)(gp + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { g[j] = a[j]; g[j + 4] = b[j]; }
        } else {
            const u16x8 r = *(const u16x8*)gp;
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = elem<TG>::from_bits16(r[j]);
        }
        if (scale) {
            const f32x4 s0 = *(const f32x4*)(scale + c * 8), s1 = *(const f32x4*)(scale + c * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { g[j] *= s0[j]; g[j + 4] *= s1[j]; }
        }
        if (relu) {
            const u16x8 yr = *(const u16x8*)(y + m * y_cs + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (!(elem<TY>::from_bits16(yr[j]) > 0.f)) g[j] = 0.f;
        }
        if (g32) {
            *(f32x4*)(g32 + vec * 8) = f32x4{g[0], g[1], g[2], g[3]};
            *(f32x4*)(g32 + vec * 8 + 4) = f32x4{g[4], g[5], g[6], g[7]};
        }
        if (gt) {
            u16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = elem<TY>::bits16(g[j]);
            *(u16x8*)(gt + vec * 8) = o;
        }
        m += dm; c += dc;
        if (c >= cv) { c -= cv; ++m; }
    }
}

template <typename TY, typename TG>
static int act_grad_t(const void* y, int y_cs, const void* gy, int gy_cs, const float* scale, long long M, int C, int relu, float* g32, void* gt,
                      step_stream_t stream) {
    if constexpr (sizeof(TY) == 2) {
        const uintptr_t al = (relu ? (uintptr_t)y : 0) | (uintptr_t)gy | (uintptr_t)gt | (uintptr_t)g32 | (uintptr_t)scale;
        if (!(C & 7) && !(y_cs & 7) && !(gy_cs & 7) && !(al & 15)) {
            const long long nvec8 = M * C / 8;
            long long blocks8 = (nvec8 + 255) / 256;
            if (blocks8 > 256LL * 32) blocks8 = 256LL * 32;
#ifdef STEP_EMUL
            if (blocks8 > 2) blocks8 = 2;                  // (host emulator: let small cases walk the grid-stride loop and its carries)
#endif
            STEP_LAUNCH((act_grad8_kernel<TY, TG>), dim3((unsigned)blocks8), dim3(256), stream, (const TY*)y, (const TG*)gy, scale, nvec8, C, y_cs, gy_cs, relu,
                        g32, (TY*)gt);
            return STEP_LAUNCH_CHECK();
        }
    }
    const long long nvec = M * C / 4;
    long long blocks = (nvec + 255) / 256;
    if (blocks > 256LL * 64) blocks = 256LL * 64;
    STEP_LAUNCH((act_grad_kernel<TY, TG>), dim3((unsigned)blocks), dim3(256), stream, (const TY*)y, (const TG*)gy, scale, nvec, C, y_cs, gy_cs, relu, g32,
                (TY*)gt);
    return STEP_LAUNCH_CHECK();
}

}  // namespace step

using namespace step;

extern "C" {

// overflow scan of the gradient arena ahead of a loss-scaled step (step_adam_flat_amp, step_sgd_flat_amp)
static void grad_scan_launch(const float* grad, long long n, float* amp_state, step_stream_t stream) {
    const long long nvec = n >> 2;
    long long blocks = (nvec + 255) / 256;
    if (blocks > 256LL * 32) blocks = 256LL * 32;
    STEP_LAUNCH(grad_scan_kernel, dim3((unsigned)blocks), dim3(256), stream, grad, nvec, amp_state);
}

static int adam_flat_launch(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n, const long long* seg_end,
                            const float* seg_lr, const float* seg_wd, int n_seg, double beta1, double beta2, double eps, int step_no,
                            long long* step_dev, float* bc_dev, float grad_scale, int zero_grad, step_stream_t stream,
                            const float* amp = nullptr) {
    if (n < 0 || (n & 3) || n_seg <= 0 || n_seg > ADAM_MAX_SEG || (!step_dev && step_no < 1)) return STEP_E_SHAPE;
    if (!(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) || !(eps >= 0.)) return STEP_E_SHAPE;
    if (step_dev && !bc_dev) return STEP_E_NULL;
    if (step_dev) STEP_LAUNCH(adam_bias_kernel, dim3(1), dim3(64), stream, step_dev, bc_dev, beta1, beta2, amp);   // (also for an empty arena: the step counts)
    if (n == 0) return step_dev ? STEP_LAUNCH_CHECK() : STEP_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !seg_end || !seg_lr || !seg_wd) return STEP_E_NULL;
    if ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) return STEP_E_ALIGN;
    // the scalars are Python doubles in torch: 1 - beta is taken in double (1.f - 0.999f is off by 1.3e-5 relative)
    const float bc1 = step_dev ? 1.f : (float)(1.0 - std::pow(beta1, (double)step_no));
    const float bc2_sqrt = step_dev ? 1.f : (float)std::sqrt(1.0 - std::pow(beta2, (double)step_no));
    const float* bcd = step_dev ? bc_dev : nullptr;
    const long long nvec = n >> 2;
    long long blocks = (nvec + 255) / 256;
    constexpr int per_cu = 64;
    if (blocks > 256LL * per_cu) blocks = 256LL * per_cu; // 64 workgroups per CU (measured: 4.6 TB/s at 16, 5.5 TB/s at 64), grid-stride beyond
    if (n_seg <= 512)
        STEP_LAUNCH((adam_flat_kernel<512>), dim3((unsigned)blocks), dim3(256), stream, param, grad, exp_avg, exp_avg_sq, nvec, seg_end,
                    seg_lr, seg_wd, n_seg, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, bc1, bc2_sqrt,
                    grad_scale, zero_grad, bcd, amp);
    else
        STEP_LAUNCH((adam_flat_kernel<ADAM_MAX_SEG>), dim3((unsigned)blocks), dim3(256), stream, param, grad, exp_avg, exp_avg_sq, nvec,
                    seg_end, seg_lr, seg_wd, n_seg, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, bc1,
                    bc2_sqrt, grad_scale, zero_grad, bcd, amp);
    return STEP_LAUNCH_CHECK();
}

int step_adam_flat(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n, const long long* seg_end,
                   const float* seg_lr, const float* seg_wd, int n_seg, double beta1, double beta2, double eps, int step_no,
                   float grad_scale, int zero_grad, step_stream_t stream) {
    return adam_flat_launch(param, grad, exp_avg, exp_avg_sq, n, seg_end, seg_lr, seg_wd, n_seg, beta1, beta2, eps, step_no, nullptr, nullptr,
                            grad_scale, zero_grad, stream);
}

int step_adam_flat_dev(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n, const long long* seg_end,
                       const float* seg_lr, const float* seg_wd, int n_seg, double beta1, double beta2, double eps, long long* step_dev,
                       float* bias_corr, float grad_scale, int zero_grad, step_stream_t stream) {
    if (!step_dev || !bias_corr) return STEP_E_NULL;
    return adam_flat_launch(param, grad, exp_avg, exp_avg_sq, n, seg_end, seg_lr, seg_wd, n_seg, beta1, beta2, eps, 0, step_dev, bias_corr,
                            grad_scale, zero_grad, stream);
}

int step_adam_flat_amp(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long long n, const long long* seg_end,
                       const float* seg_lr, const float* seg_wd, int n_seg, double beta1, double beta2, double eps, long long* step_dev,
                       float* bias_corr, float grad_scale, int zero_grad, float* amp_state, float growth_factor, float backoff_factor,
                       int growth_interval, step_stream_t stream) {
    if (!step_dev || !bias_corr || !amp_state) return STEP_E_NULL;
    if (n < 0 || (n & 3) || growth_interval < 1 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f)) return STEP_E_SHAPE;
    if (n > 0) {
        if (!grad) return STEP_E_NULL;
        if ((uintptr_t)grad & 15) return STEP_E_ALIGN;
        grad_scan_launch(grad, n, amp_state, stream);
    }
    const int rc = adam_flat_launch(param, grad, exp_avg, exp_avg_sq, n, seg_end, seg_lr, seg_wd, n_seg, beta1, beta2, eps, 0, step_dev, bias_corr,
                                    grad_scale, zero_grad, stream, amp_state);
    if (rc) return rc;
    STEP_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), stream, amp_state, growth_factor, backoff_factor, growth_interval);
    return STEP_LAUNCH_CHECK();
}

// every argument is checked before the first launch: a refused call has written nothing
static int sgd_flat_check(float* param, float* grad, float* buf, long long n, const long long* seg_end, const float* seg_lr,
                          const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov, int step_no,
                          const long long* step_dev) {
    if (n < 0 || (n & 3) || n_seg <= 0 || n_seg > ADAM_MAX_SEG || (!step_dev && step_no < 1)) return STEP_E_SHAPE;
    if (!(momentum >= 0.) || !std::isfinite(momentum) || !std::isfinite(dampening)) return STEP_E_SHAPE;
    if (nesterov && (momentum <= 0. || dampening != 0.)) return STEP_E_SHAPE;     // torch: "Nesterov momentum requires a momentum and zero dampening"
    if (n == 0) return STEP_OK;
    if (!param || !grad || (momentum != 0. && !buf) || !seg_end || !seg_lr || !seg_wd) return STEP_E_NULL;
    if ((((uintptr_t)param) | ((uintptr_t)grad) | (momentum != 0. ? (uintptr_t)buf : 0)) & 15) return STEP_E_ALIGN;
    return STEP_OK;
}

static int sgd_flat_launch(float* param, float* grad, float* buf, long long n, const long long* seg_end, const float* seg_lr,
                           const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov, int step_no,
                           long long* step_dev, float grad_scale, int zero_grad, step_stream_t stream, const float* amp = nullptr) {
    if (n > 0) {
        const long long nvec = n >> 2;
        long long blocks = (nvec + 255) / 256;
        constexpr int per_cu = 64;
        if (blocks > 256LL * per_cu) blocks = 256LL * per_cu;   // as the Adam pass: 64 workgroups per CU, grid-stride beyond
        // the scalars are Python doubles in torch: 1 - dampening is taken in double
        const float mu = (float)momentum, omd = (float)(1.0 - dampening);
        const int first = step_no == 1;
#define STEP_SGD_LAUNCH(MAXSEG, MOM)                                                                                                  \
    STEP_LAUNCH((sgd_flat_kernel<MAXSEG, MOM>), dim3((unsigned)blocks), dim3(256), stream, param, grad, buf, nvec, seg_end, seg_lr, seg_wd, \
                n_seg, mu, omd, nesterov, first, grad_scale, zero_grad, (const long long*)step_dev, amp)
        if (momentum != 0.) {
            if (n_seg <= 512) STEP_SGD_LAUNCH(512, true); else STEP_SGD_LAUNCH(ADAM_MAX_SEG, true);
        } else {
            if (n_seg <= 512) STEP_SGD_LAUNCH(512, false); else STEP_SGD_LAUNCH(ADAM_MAX_SEG, false);
        }
#undef STEP_SGD_LAUNCH
    }
    if (step_dev) STEP_LAUNCH(sgd_count_kernel, dim3(1), dim3(64), stream, step_dev, amp);   // (also for an empty arena: the step counts)
    return (n > 0 || step_dev) ? STEP_LAUNCH_CHECK() : STEP_OK;
}

int step_sgd_flat(float* param, float* grad, float* momentum_buf, long long n, const long long* seg_end, const float* seg_lr,
                  const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov, int step_no, float grad_scale,
                  int zero_grad, step_stream_t stream) {
    const int rc = sgd_flat_check(param, grad, momentum_buf, n, seg_end, seg_lr, seg_wd, n_seg, momentum, dampening, nesterov, step_no, nullptr);
    if (rc) return rc;
    return sgd_flat_launch(param, grad, momentum_buf, n, seg_end, seg_lr, seg_wd, n_seg, momentum, dampening, nesterov, step_no, nullptr,
                           grad_scale, zero_grad, stream);
}

int step_sgd_flat_dev(float* param, float* grad, float* momentum_buf, long long n, const long long* seg_end, const float* seg_lr,
                      const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov, long long* step_dev,
                      float grad_scale, int zero_grad, step_stream_t stream) {
    if (!step_dev) return STEP_E_NULL;
    const int rc = sgd_flat_check(param, grad, momentum_buf, n, seg_end, seg_lr, seg_wd, n_seg, momentum, dampening, nesterov, 0, step_dev);
    if (rc) return rc;
    return sgd_flat_launch(param, grad, momentum_buf, n, seg_end, seg_lr, seg_wd, n_seg, momentum, dampening, nesterov, 0, step_dev,
                           grad_scale, zero_grad, stream);
}

int step_sgd_flat_amp(float* param, float* grad, float* momentum_buf, long long n, const long long* seg_end, const float* seg_lr,
                      const float* seg_wd, int n_seg, double momentum, double dampening, int nesterov, long long* step_dev,
                      float grad_scale, int zero_grad, float* amp_state, float growth_factor, float backoff_factor, int growth_interval,
                      step_stream_t stream) {
    if (!step_dev || !amp_state) return STEP_E_NULL;
    if (growth_interval < 1 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f)) return STEP_E_SHAPE;
    int rc = sgd_flat_check(param, grad, momentum_buf, n, seg_end, seg_lr, seg_wd, n_seg, momentum, dampening, nesterov, 0, step_dev);
    if (rc) return rc;
    if (n > 0) grad_scan_launch(grad, n, amp_state, stream);
    rc = sgd_flat_launch(param, grad, momentum_buf, n, seg_end, seg_lr, seg_wd, n_seg, momentum, dampening, nesterov, 0, step_dev, grad_scale,
                         zero_grad, stream, amp_state);
    if (rc) return rc;
    STEP_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), stream, amp_state, growth_factor, backoff_factor, growth_interval);
    return STEP_LAUNCH_CHECK();
}

// every argument is checked before the first launch: a refused call has written nothing (as sgd_flat_check)
static int grad_wire_check(int wire_dtype, const float* grad, const float* residual, const void* wire, long long n) {
    if (wire_dtype == STEP_F16 || wire_dtype == STEP_F32) return STEP_E_UNSUPPORTED;     // one wire format: bfloat16
    if (wire_dtype != STEP_BF16) return STEP_E_DTYPE;
    if (n < 0) return STEP_E_SHAPE;
    if (n == 0) return STEP_OK;
    if (!grad || !wire) return STEP_E_NULL;
    if ((((uintptr_t)grad) | ((uintptr_t)residual)) & 3 || ((uintptr_t)wire & 1)) return STEP_E_ALIGN;
    return STEP_OK;
}

// 8 workgroups per CU are resident at once (32 wavefronts): one pass of the grid covers 2^22 elements of the vector body, the 44.4 M of
// the full arena take 11 passes of the grid-stride loop
static unsigned grad_wire_blocks(long long items) {
    long long blocks = (items + 255) / 256;
    if (blocks > 256LL * 8) blocks = 256LL * 8;
#ifdef STEP_EMUL
    if (blocks > 2) blocks = 2;                            // (host emulator: let small cases walk the grid-stride loop)
#endif
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

int step_grad_pack16(int wire_dtype, const float* grad, float* residual, void* wire, long long n, float pre_scale, step_stream_t stream) {
    const int rc = grad_wire_check(wire_dtype, grad, residual, wire, n);
    if (rc || n == 0) return rc;
    const bool vec = !((((uintptr_t)grad) | ((uintptr_t)residual) | ((uintptr_t)wire)) & 15);
    const dim3 grid(grad_wire_blocks(vec ? (n + 7) >> 3 : n));
    unsigned short* w = (unsigned short*)wire;
    if (residual) {
        if (vec) STEP_LAUNCH((grad_pack16_kernel<true, true>), grid, dim3(256), stream, grad, residual, w, n, pre_scale);
        else STEP_LAUNCH((grad_pack16_kernel<true, false>), grid, dim3(256), stream, grad, residual, w, n, pre_scale);
    } else {
        if (vec) STEP_LAUNCH((grad_pack16_kernel<false, true>), grid, dim3(256), stream, grad, residual, w, n, pre_scale);
        else STEP_LAUNCH((grad_pack16_kernel<false, false>), grid, dim3(256), stream, grad, residual, w, n, pre_scale);
    }
    return STEP_LAUNCH_CHECK();
}

int step_grad_unpack16(int wire_dtype, const void* wire, float* grad, long long n, step_stream_t stream) {
    const int rc = grad_wire_check(wire_dtype, grad, nullptr, wire, n);
    if (rc || n == 0) return rc;
    const bool vec = !((((uintptr_t)grad) | ((uintptr_t)wire)) & 15);
    const dim3 grid(grad_wire_blocks(vec ? (n + 7) >> 3 : n));
    const unsigned short* w = (const unsigned short*)wire;
    if (vec) STEP_LAUNCH((grad_unpack16_kernel<true>), grid, dim3(256), stream, w, grad, n);
    else STEP_LAUNCH((grad_unpack16_kernel<false>), grid, dim3(256), stream, w, grad, n);
    return STEP_LAUNCH_CHECK();
}

static long long grad_norm_chunks(long long n) { return (n + GN_CHUNK - 1) / GN_CHUNK; }

size_t step_grad_norm_workspace_bytes(long long n, int n_seg) {
    if (n < 0 || n_seg <= 0 || n_seg > ADAM_MAX_SEG) return 0;
    return (size_t)(grad_norm_chunks(n) + n_seg) * sizeof(double);       // slot c + s: chunk c's part of segment s
}

int step_grad_norm_flat(const float* grad, long long n, const long long* seg_end, int n_seg, float grad_scale, const float* amp_state,
                        float max_norm, void* workspace, size_t workspace_bytes, float* seg_norm, float* stats, step_stream_t stream) {
    if (!(max_norm > 0.f) || n < 0 || (n & 3) || n_seg <= 0 || n_seg > ADAM_MAX_SEG) return STEP_E_SHAPE;
    if (n == 0) return STEP_OK;
    if (!grad || !seg_end || !workspace || !stats) return STEP_E_NULL;
    if (((uintptr_t)grad & 15) || ((uintptr_t)workspace & 7)) return STEP_E_ALIGN;
    if (workspace_bytes < step_grad_norm_workspace_bytes(n, n_seg)) return STEP_E_SHAPE;
    long long blocks = grad_norm_chunks(n);
    if (blocks > 256LL * 8) blocks = 256LL * 8;             // 8 workgroups per CU resident at once, grid-stride over the chunks beyond
#ifdef STEP_EMUL
    if (blocks > 2) blocks = 2;                            // (host emulator: let small cases walk the grid-stride loop)
#endif
    if (n_seg <= 512)
        STEP_LAUNCH((grad_norm_partial_kernel<512>), dim3((unsigned)blocks), dim3(256), stream, grad, n, seg_end, n_seg, (double*)workspace);
    else
        STEP_LAUNCH((grad_norm_partial_kernel<ADAM_MAX_SEG>), dim3((unsigned)blocks), dim3(256), stream, grad, n, seg_end, n_seg,
                    (double*)workspace);
    STEP_LAUNCH(grad_norm_finish_kernel, dim3(1), dim3(GN_FIN_THREADS), stream, n, seg_end, n_seg, (const double*)workspace, grad_scale,
                amp_state, max_norm, seg_norm, stats);
    return STEP_LAUNCH_CHECK();
}

int step_grad_clip_flat(float* grad, long long n, const float* stats, step_stream_t stream) {
    if (n < 0 || (n & 3)) return STEP_E_SHAPE;
    if (n == 0) return STEP_OK;
    if (!grad || !stats) return STEP_E_NULL;
    if ((uintptr_t)grad & 15) return STEP_E_ALIGN;
    const long long nvec = n >> 2;
    long long blocks = (nvec + 255) / 256;
    if (blocks > 256LL * 32) blocks = 256LL * 32;           // as grad_scan: a pure streaming pass
#ifdef STEP_EMUL
    if (blocks > 2) blocks = 2;
#endif
    STEP_LAUNCH(grad_clip_kernel, dim3((unsigned)blocks), dim3(256), stream, grad, nvec, stats);
    return STEP_LAUNCH_CHECK();
}

int step_lr_schedule(int kind, long long* iter_dev, const double* base_lr, float* seg_lr, int n_seg, const long long* milestones,
                     int n_milestones, long long warmup_iters, double warmup_factor, double p0, double p1, step_stream_t stream) {
    if (kind != STEP_LR_COSINE && kind != STEP_LR_STEP) return STEP_E_SHAPE;
    if (n_seg <= 0 || n_seg > ADAM_MAX_SEG || warmup_iters < 0) return STEP_E_SHAPE;
    if (n_milestones < (kind == STEP_LR_COSINE ? 2 : 0) || n_milestones > LR_MAX_MS) return STEP_E_SHAPE;
    if (!iter_dev || !base_lr || !seg_lr || (n_milestones > 0 && !milestones)) return STEP_E_NULL;
    STEP_LAUNCH(lr_schedule_kernel, dim3(1), dim3(256), stream, kind, iter_dev, base_lr, seg_lr, n_seg, milestones, n_milestones, warmup_iters,
                warmup_factor, p0, p1);
    return STEP_LAUNCH_CHECK();
}

int step_act_grad(int dtype, const void* y, int y_cstride, int gy_dtype, const void* gy, int gy_cstride, const float* scale, long long M, int C,
                  int relu, float* g32, void* g_act, step_stream_t stream) {
    if (M < 0 || C <= 0) return STEP_E_SHAPE;
    if (y_cstride == 0) y_cstride = C;
    if (gy_cstride == 0) gy_cstride = C;
    if (y_cstride < C || gy_cstride < C) return STEP_E_SHAPE;
    if ((C & 3) || (y_cstride & 3) || (gy_cstride & 3)) return STEP_E_UNSUPPORTED;     // 4-channel vectors
    {
        const int yb = dtype == STEP_F32 ? 16 : 8, gb = gy_dtype == STEP_F32 ? 16 : 8;
        if ((relu && ((uintptr_t)y & (yb - 1))) || ((uintptr_t)gy & (gb - 1)) || ((uintptr_t)g32 & 15) || ((uintptr_t)g_act & (yb - 1)) ||
            ((uintptr_t)scale & 15))
            return STEP_E_ALIGN;
    }
    if (M == 0) return STEP_OK;
    if (!gy || (relu && !y) || (!g32 && !g_act)) return STEP_E_NULL;
    if (gy_dtype != STEP_F32 && gy_dtype != dtype) return STEP_E_DTYPE;
    const bool gf = gy_dtype == STEP_F32;
    switch (dtype) {
        case STEP_F32: return act_grad_t<float, float>(y, y_cstride, gy, gy_cstride, scale, M, C, relu, g32, g_act, stream);
        case STEP_BF16: return gf ? act_grad_t<bf16_t, float>(y, y_cstride, gy, gy_cstride, scale, M, C, relu, g32, g_act, stream)
                                  : act_grad_t<bf16_t, bf16_t>(y, y_cstride, gy, gy_cstride, scale, M, C, relu, g32, g_act, stream);
        case STEP_F16: return gf ? act_grad_t<f16_t, float>(y, y_cstride, gy, gy_cstride, scale, M, C, relu, g32, g_act, stream)
                                 : act_grad_t<f16_t, f16_t>(y, y_cstride, gy, gy_cstride, scale, M, C, relu, g32, g_act, stream);
    }
    return STEP_E_DTYPE;
}

}  // extern "C"
