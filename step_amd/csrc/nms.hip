// step_amd/csrc/nms.hip -- batched greedy NMS for gfx950, bit-exact with the reference CPU op.
//
// Replaces  external/maskrcnn_benchmark/csrc/cpu/nms_cpu.cpp:29-89 (the operator every reference
// script actually reaches: test.py:158-161,192 / train.py:513-515,547 / demo.py:124-126,158 move the
// boxes to the CPU first) and csrc/cuda/nms.cu:47-155 (64x64 bit-mask tiles + a serial host
// reduction behind a blocking D2H copy).
//
// STEP calls nms once per (step, clip, class) on <= 34..109 middle-frame boxes: 180*B tiny serial
// CPU calls per batch.  Here all groups go in ONE launch:
//   * kmax <= 64  : one 64-lane wavefront per group, boxes live in registers, the greedy scan is a
//                   loop of cross-lane broadcasts -- no LDS, no global scratch, no host round trip;
//   * kmax  > 64  : one 256-thread workgroup per group with a global scratch rank table (step_nms_batched), or with all state in LDS
//                   (step_detect_nms up to 1024 tubes: detect_nms_block_kernel).
// Arithmetic: "+1" areas, IoU = inter / (area_i + area_j - inter) with every operation rounded
// separately (__f*_rn: no FMA contraction), suppress when IoU >= threshold (nms_cpu.cpp:84 -- the
// CUDA op uses '>', nms.cu:84; parity target is the CPU op), ties in score broken by lower index.
//
// Behind it in this file: the rows of the evaluation loop (detect_compact), their cross-class merge (detect_merge) and the frame-mAP
// evaluation of those rows (round_sig4, eval_match, eval_ap: external/ActivityNet/Evaluation restated in float64).
#include "common.h"

#pragma clang fp contract(off)

namespace step {

__device__ __forceinline__ float box_area(float x1, float y1, float x2, float y2) {
    return __fmul_rn(__fadd_rn(__fsub_rn(x2, x1), 1.f), __fadd_rn(__fsub_rn(y2, y1), 1.f));  // nms_cpu.cpp:46
}
// fp64 boxes (the reference dispatches AT_DISPATCH_FLOATING_TYPES, nms_cpu.cpp:95): the same operations in double, each rounded
// separately (this file is compiled with fp contraction off); the threshold stays the operator's float argument, promoted in
// `ovr >= threshold` as in nms_cpu_kernel<double>.
__device__ __forceinline__ double box_area(double x1, double y1, double x2, double y2) {
    const double w = (x2 - x1) + 1.0, h = (y2 - y1) + 1.0;
    return w * h;
}
__device__ __forceinline__ bool iou_ge(double ix1, double iy1, double ix2, double iy2, double iarea, double jx1, double jy1,
                                       double jx2, double jy2, double jarea, float thr) {
    const double xx1 = fmax(ix1, jx1), yy1 = fmax(iy1, jy1);
    const double xx2 = fmin(ix2, jx2), yy2 = fmin(iy2, jy2);
    const double w = fmax(0.0, (xx2 - xx1) + 1.0);
    const double h = fmax(0.0, (yy2 - yy1) + 1.0);
    const double inter = w * h;
    const double ovr = inter / ((iarea + jarea) - inter);
    return ovr >= (double)thr;
}

// i = the kept (higher score) box, j = the candidate.  nms_cpu.cpp:73-84
__device__ __forceinline__ bool iou_ge(float ix1, float iy1, float ix2, float iy2, float iarea, float jx1, float jy1,
                                       float jx2, float jy2, float jarea, float thr) {
    float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
    float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
    float w = fmaxf(0.f, __fadd_rn(__fsub_rn(xx2, xx1), 1.f));
    float h = fmaxf(0.f, __fadd_rn(__fsub_rn(yy2, yy1), 1.f));
    float inter = __fmul_rn(w, h);
    float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(iarea, jarea), inter));
    return ovr >= thr;
}

// Score order: descending, ties by lower index.  NaN scores sort FIRST (torch's sort, which the reference uses at
// nms_cpu.cpp:50, treats NaN as the largest value); without this rule NaNs compare false both ways, ranks collide and
// the rank -> lane lookup below would be undefined.
template <typename F>
__device__ __forceinline__ bool score_before(F sj, int j, F s, int i) {
    const bool nj = sj != sj, ni = s != s;
    if (nj || ni) return nj && (!ni || j < i);
    return sj > s || (sj == s && j < i);
}

// One wavefront per group, n <= 64.
template <typename F>
__global__ void nms_wave_kernel(const F* __restrict__ boxes, const F* __restrict__ scores,
                                const int32_t* __restrict__ counts, int kmax, float thr, uint8_t* __restrict__ keep) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;  // blockDim.x == 64
    const int n = min(counts[g], kmax);
    const bool valid = lane < n;
    F x1 = 0, y1 = 0, x2 = 0, y2 = 0, s = 0;
    if (valid) {
        const F* b = boxes + ((size_t)g * kmax + lane) * 4;
        x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3];
        s = scores[(size_t)g * kmax + lane];
    }
    const F area = box_area(x1, y1, x2, y2);
    // stable descending rank (ties: lower index first)
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        F sj = __shfl(s, j);
        rank += score_before(sj, j, s, lane) ? 1 : 0;
    }
    bool suppressed = false;
    for (int r = 0; r < n; ++r) {
        unsigned long long m = __ballot(valid && rank == r);
        int i = __builtin_ctzll(m);  // exactly one lane has rank r
        unsigned long long sm = __ballot(suppressed);
        F bx1 = __shfl(x1, i), by1 = __shfl(y1, i), bx2 = __shfl(x2, i), by2 = __shfl(y2, i);
        F barea = __shfl(area, i);
        if ((sm >> i) & 1ull) continue;  // wave-uniform
        if (valid && !suppressed && rank > r && iou_ge(bx1, by1, bx2, by2, barea, x1, y1, x2, y2, area, thr))
            suppressed = true;
    }
    if (lane < kmax) keep[(size_t)g * kmax + lane] = (valid && !suppressed) ? 1 : 0;
}

// The evaluation loop of test.py:157-198 for one refinement iteration as ONE launch: wavefront (b, c) takes clip b's tubes (slot j =
// lane), masks them with score > conf (test.py:180), clamps their middle-frame boxes the way valid_tubes does (tube_utils.py:59-92:
// clip to [0, width] x [0, height], boxes under 3 px become the whole frame) and runs the greedy NMS among the masked ones -- the
// reference compacts them first, keeping their order, so score ties still go to the lower original slot.  keep[b][c][j] marks the
// survivors at their ORIGINAL slots.  n <= 64 tubes per clip.
__global__ void detect_nms_wave_kernel(const float* __restrict__ prob, long long prob_stride, int NC, const float* __restrict__ loc,
                                       long long loc_stride, const int32_t* __restrict__ tube_start, const int32_t* __restrict__ tube_count,
                                       int kmax, float conf, float thr, float width, float height, uint8_t* __restrict__ keep,
                                       float* __restrict__ boxes_out) {
    const int b = blockIdx.x / NC, c = blockIdx.x % NC;
    const int lane = threadIdx.x;
    const int n = min(tube_count[b], kmax);
    const long long tube = (long long)tube_start[b] + lane;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, s = 0.f;
    bool valid = false;
    if (lane < n) {
        const float* bx = loc + tube * loc_stride;
        x1 = fmaxf(0.f, bx[0]); y1 = fmaxf(0.f, bx[1]); x2 = fminf(width, bx[2]); y2 = fminf(height, bx[3]);
        // np.maximum / np.minimum PROPAGATE a NaN (fmaxf / fminf drop it), and a NaN coordinate then fails the `<` test of
        // valid_tubes: the reference turns a box with any NaN coordinate into the whole frame
        const bool nan_in = (bx[0] != bx[0]) || (bx[1] != bx[1]) || (bx[2] != bx[2]) || (bx[3] != bx[3]);
        if (nan_in || !((x1 < __fsub_rn(x2, 2.f)) && (y1 < __fsub_rn(y2, 2.f)))) { x1 = 0.f; y1 = 0.f; x2 = width; y2 = height; }
        s = prob[tube * prob_stride + c];
        valid = s > conf;
        if (c == 0 && boxes_out) {
            float* o = boxes_out + tube * 4;
            o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
        }
    }
    const float area = box_area(x1, y1, x2, y2);
    const unsigned long long vm = __ballot(valid);
    int rank = 0;                                              // descending score among the masked tubes, ties: lower slot first
    for (int j = 0; j < n; ++j) {
        const float sj = __shfl(s, j);
        rank += (((vm >> j) & 1ull) && score_before(sj, j, s, lane)) ? 1 : 0;
    }
    const int nv = __builtin_popcountll(vm);
    bool suppressed = false;
    for (int r = 0; r < nv; ++r) {
        const unsigned long long m = __ballot(valid && rank == r);
        const int i = __builtin_ctzll(m);                    // exactly one masked lane has rank r
        const unsigned long long sm = __ballot(suppressed);
        const float bx1 = __shfl(x1, i), by1 = __shfl(y1, i), bx2 = __shfl(x2, i), by2 = __shfl(y2, i);
        const float barea = __shfl(area, i);
        if ((sm >> i) & 1ull) continue;                       // wave-uniform
        if (valid && !suppressed && rank > r && iou_ge(bx1, by1, bx2, by2, barea, x1, y1, x2, y2, area, thr)) suppressed = true;
    }
    if (lane < kmax) keep[((size_t)b * NC + c) * kmax + lane] = (valid && !suppressed) ? 1 : 0;
}

// The same contract for 64 < kmax <= STEP_DETECT_TUBES_MAX: one 256-thread workgroup per (clip, class), all state in LDS (28.3 KiB), no
// global scratch.  Thread t owns slots t, t + 256, t + 512, t + 768 (the load and clamp of the wave kernel restated, not shared: DESIGN
// 3.14).
//   1. load / clamp / mask; the slot-order scores and the "masked" bitmap (one ballot per 64 slots) go to LDS; an unmasked slot's flag is
//      cleared here.  A group with no masked slot leaves after this.
//   2. rank of every masked slot by counting against LDS broadcasts of the MASKED scores only (the walk over the set bits is uniform for
//      the workgroup); box, area and slot go to LDS at position rank: the list in NMS order.
//   3. the scan, as in detect_merge_kernel: `alive` is a bitmap in rank order; the next kept box is the first set bit past the previous
//      one (16 words: one ballot + ctz, every wave finds the same one); the four waves take the later words round-robin, lane = position,
//      and clear the suppressed bits with ONE plain 64-bit store of the wave's ballot per word (a word belongs to one wave).  The search
//      reads only bits at or past the leader, the scan clears only bits past it: ONE barrier per KEPT box.
//   4. keep[slot_of[p]] = alive bit p.  Every slot < kmax is written exactly once (here or in 1).
#define DN_SLOTS STEP_DETECT_TUBES_MAX
#define DN_WORDS (DN_SLOTS / 64)
#define DN_PER_THREAD (DN_SLOTS / 256)
__global__ __launch_bounds__(256) void detect_nms_block_kernel(const float* __restrict__ prob, long long prob_stride, int NC,
                                                               const float* __restrict__ loc, long long loc_stride,
                                                               const int32_t* __restrict__ tube_start, const int32_t* __restrict__ tube_count,
                                                               int kmax, float conf, float thr, float width, float height,
                                                               uint8_t* __restrict__ keep, float* __restrict__ boxes_out) {
    __shared__ float ssc[DN_SLOTS];                            // scores, SLOT order
    __shared__ float rx1[DN_SLOTS], ry1[DN_SLOTS], rx2[DN_SLOTS], ry2[DN_SLOTS], rar[DN_SLOTS];   // boxes and areas, RANK order
    __shared__ int32_t slot_of[DN_SLOTS];                      // rank -> slot
    __shared__ unsigned long long masked[DN_WORDS];            // bit (j & 63) of word (j >> 6): slot j has score > conf
    __shared__ unsigned long long alive[DN_WORDS];             // the same for list position p: not suppressed (yet)
    const int b = blockIdx.x / NC, c = blockIdx.x % NC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(tube_count[b], kmax);
    const long long t0 = tube_start[b];
    uint8_t* kp = keep + ((size_t)b * NC + c) * kmax;
    const int swords = (n + 63) >> 6;                          // words of `masked` that hold a slot

    float x1[DN_PER_THREAD], y1[DN_PER_THREAD], x2[DN_PER_THREAD], y2[DN_PER_THREAD], s[DN_PER_THREAD];
    bool valid[DN_PER_THREAD];
#pragma unroll
    for (int u = 0; u < DN_PER_THREAD; ++u) {
        const int j = tid + 256 * u;                           // word (j >> 6) = wave + 4 * u: written by this wave alone
        x1[u] = 0.f; y1[u] = 0.f; x2[u] = 0.f; y2[u] = 0.f; s[u] = 0.f;
        valid[u] = false;
        if (j < n) {
            const long long tube = t0 + j;
            const float* bx = loc + tube * loc_stride;
            x1[u] = fmaxf(0.f, bx[0]); y1[u] = fmaxf(0.f, bx[1]); x2[u] = fminf(width, bx[2]); y2[u] = fminf(height, bx[3]);
            // (NaN coordinates: see detect_nms_wave_kernel)
            const bool nan_in = (bx[0] != bx[0]) || (bx[1] != bx[1]) || (bx[2] != bx[2]) || (bx[3] != bx[3]);
            if (nan_in || !((x1[u] < __fsub_rn(x2[u], 2.f)) && (y1[u] < __fsub_rn(y2[u], 2.f)))) { x1[u] = 0.f; y1[u] = 0.f; x2[u] = width; y2[u] = height; }
            s[u] = prob[tube * prob_stride + c];
            valid[u] = s[u] > conf;
            if (c == 0 && boxes_out) {
                float* o = boxes_out + tube * 4;
                o[0] = x1[u]; o[1] = y1[u]; o[2] = x2[u]; o[3] = y2[u];
            }
            ssc[j] = s[u];
        }
        if (64 * (wave + 4 * u) < n) {                         // wave-uniform
            const unsigned long long m = __ballot(valid[u]);
            if (lane == 0) masked[wave + 4 * u] = m;
        }
        if (j < kmax && !valid[u]) kp[j] = 0;
    }
    __syncthreads();

    int nv = 0;
    int rank[DN_PER_THREAD];
#pragma unroll
    for (int u = 0; u < DN_PER_THREAD; ++u) rank[u] = 0;
    for (int w = 0; w < swords; ++w) {
        unsigned long long m = masked[w];
        nv += __builtin_popcountll(m);
        while (m) {                                            // uniform for the workgroup
            const int j = 64 * w + __builtin_ctzll(m);
            m &= m - 1ull;
            const float sj = ssc[j];
#pragma unroll
            for (int u = 0; u < DN_PER_THREAD; ++u) rank[u] += score_before(sj, j, s[u], tid + 256 * u) ? 1 : 0;
        }
    }
    if (nv == 0) return;                                       // nothing masked: the flags are cleared
#pragma unroll
    for (int u = 0; u < DN_PER_THREAD; ++u)
        if (valid[u]) {                                        // ranks of the masked slots are a permutation of 0 .. nv - 1
            const int r = rank[u];
            rx1[r] = x1[u]; ry1[r] = y1[u]; rx2[r] = x2[u]; ry2[r] = y2[u];
            rar[r] = box_area(x1[u], y1[u], x2[u], y2[u]);
            slot_of[r] = tid + 256 * u;
        }
    const int nwords = (nv + 63) >> 6;
    if (tid < nwords) alive[tid] = (64 * tid + 64 <= nv) ? ~0ull : ((1ull << (nv - 64 * tid)) - 1ull);
    __syncthreads();

    for (int from = 0; from < nv;) {
        // the next kept box: the first set bit at or past `from`
        const int wf = from >> 6;
        unsigned long long word = (lane >= wf && lane < nwords) ? alive[lane] : 0ull;
        if (lane == wf) word &= ~0ull << (from & 63);
        const unsigned long long found = __ballot(word != 0ull);
        if (!found) break;
        const int wL = __builtin_ctzll(found);
        const int L = 64 * wL + __builtin_ctzll(__shfl(word, wL));
        const float lx1 = rx1[L], ly1 = ry1[L], lx2 = rx2[L], ly2 = ry2[L], larea = rar[L];
        for (int w = wL + wave; w < nwords; w += 4) {
            const unsigned long long cur = alive[w];
            const unsigned long long later = w == wL ? (((L & 63) == 63) ? 0ull : (~0ull << ((L & 63) + 1))) : ~0ull;
            if ((cur & later) == 0ull) continue;               // wave-uniform
            const int p = 64 * w + lane;
            bool sup = ((cur & later) >> lane) & 1ull;
            if (sup) sup = iou_ge(lx1, ly1, lx2, ly2, larea, rx1[p], ry1[p], rx2[p], ry2[p], rar[p], thr);
            const unsigned long long m = __ballot(sup);
            if (m && lane == 0) alive[w] = cur & ~m;
        }
        from = L + 1;
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < DN_PER_THREAD; ++u) {
        const int p = tid + 256 * u;
        if (p < nv) kp[slot_of[p]] = (uint8_t)((alive[p >> 6] >> (p & 63)) & 1ull);
    }
}

// One 256-thread workgroup per group, any n.  scratch: order int32[G*kmax], sup uint8[G*kmax].
template <typename F>
__global__ void nms_block_kernel(const F* __restrict__ boxes, const F* __restrict__ scores,
                                 const int32_t* __restrict__ counts, int kmax, float thr, uint8_t* __restrict__ keep,
                                 int32_t* order_all, uint8_t* sup_all) {
    const int g = blockIdx.x;
    const int n = min(counts[g], kmax);
    const F* B = boxes + (size_t)g * kmax * 4;
    const F* S = scores + (size_t)g * kmax;
    int32_t* order = order_all + (size_t)g * kmax;
    uint8_t* sup = sup_all + (size_t)g * kmax;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const F s = S[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            F sj = S[j];
            rank += score_before(sj, j, s, i) ? 1 : 0;
        }
        order[rank] = i;
        sup[i] = 0;
    }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
        const int i = order[r];
        const bool isup = sup[i] != 0;  // uniform: written before the last barrier
        if (!isup) {
            const F ix1 = B[4 * i], iy1 = B[4 * i + 1], ix2 = B[4 * i + 2], iy2 = B[4 * i + 3];
            const F iarea = box_area(ix1, iy1, ix2, iy2);
            for (int q = r + 1 + threadIdx.x; q < n; q += blockDim.x) {
                const int j = order[q];
                if (sup[j]) continue;
                const F jx1 = B[4 * j], jy1 = B[4 * j + 1], jx2 = B[4 * j + 2], jy2 = B[4 * j + 3];
                if (iou_ge(ix1, iy1, ix2, iy2, iarea, jx1, jy1, jx2, jy2, box_area(jx1, jy1, jx2, jy2), thr)) sup[j] = 1;
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < kmax; i += blockDim.x) keep[(size_t)g * kmax + i] = (i < n && !sup[i]) ? 1 : 0;
}

template <typename F>
static int nms_batched_t(const F* boxes, const F* scores, const int32_t* counts, int G, int kmax, float threshold, uint8_t* keep, void* scratch,
                         step_stream_t stream) {
    if (G < 0 || kmax < 0) return STEP_E_SHAPE;
    if (G == 0 || kmax == 0) return STEP_OK;
    if (!boxes || !scores || !counts || !keep) return STEP_E_NULL;
    if (kmax <= 64) {
        STEP_LAUNCH((nms_wave_kernel<F>), dim3(G), dim3(64), stream, boxes, scores, counts, kmax, threshold, keep);
    } else {
        if (!scratch) return STEP_E_NULL;
        int32_t* order = (int32_t*)scratch;
        uint8_t* sup = (uint8_t*)scratch + (size_t)G * kmax * 4;
        STEP_LAUNCH((nms_block_kernel<F>), dim3(G), dim3(256), stream, boxes, scores, counts, kmax, threshold, keep, order, sup);
    }
    return STEP_LAUNCH_CHECK();
}

// detect_compact_kernel -- the rows test.py:196-204 appends after the NMS of an iteration, for ALL iterations and clips in one launch: one
// 256-thread workgroup per (iteration, clip) walks its NC x kmax keep flags in row-major order (classes ascending, kept tubes in ascending
// original order: the reference's row order), numbers the set flags with a ballot prefix and writes box / [W,H,W,H], score, class, tube of
// row r to slot g * cap + r of its own fixed-capacity segment (cap = NC * kmax) -- no prefix sum across workgroups, the host reads the
// I x B counts once and slices.  (Before: nonzero + index + cat + gather + bincount, ~25 launches and two host synchronisations per step.)
struct DetectCompactParams {
    const float* boxes[STEP_DETECT_ITERS_MAX];
    const float* scores[STEP_DETECT_ITERS_MAX];
    long long score_stride[STEP_DETECT_ITERS_MAX];
    const uint8_t* keep; const int32_t* start;
    int B, NC, kmax;
    float w, h;
    float* out_boxes; float* out_scores; long long* out_cls; long long* out_tube; int32_t* counts;
};
__global__ __launch_bounds__(256) void detect_compact_kernel(DetectCompactParams p) {
    __shared__ int wsum[4];
    const int g = blockIdx.x, it = g / p.B, b = g % p.B;
    const int F = p.NC * p.kmax;
    const uint8_t* kp = p.keep + (size_t)g * F;
    const float* bx = p.boxes[it];
    const float* sc = p.scores[it];
    const long long ss = p.score_stride[it];
    const int t0 = F > 0 ? p.start[b] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int f0 = 0; f0 < F; f0 += 256) {
        const int f = f0 + (int)threadIdx.x;
        const bool on = f < F && kp[f] != 0;
        const unsigned long long m = __ballot(on);
        const int before = __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __builtin_popcountll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (on) {
            const int c = f / p.kmax, j = f - c * p.kmax;
            const size_t row = (size_t)g * F + off + before;
            const float* bb = bx + (size_t)(t0 + j) * 4;
            p.out_boxes[row * 4 + 0] = bb[0] / p.w; p.out_boxes[row * 4 + 1] = bb[1] / p.h;
            p.out_boxes[row * 4 + 2] = bb[2] / p.w; p.out_boxes[row * 4 + 3] = bb[3] / p.h;
            p.out_scores[row] = sc[(size_t)(t0 + j) * ss + c];
            p.out_cls[row] = c;
            p.out_tube[row] = j;
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) p.counts[g] = base;
}

// detect_merge_kernel -- the cross-class merge of demo.py:176-198 on the rows of detect_compact_kernel, all (iteration, clip) groups in one
// launch: one 256-thread workgroup per group.  List position p is row order[p] of the group's segment (identity without `order`).
//   * the "not yet flagged" state of the reference's `flag` list is a bitmap in LDS, one 64-bit word per 64 consecutive list positions;
//   * the serial loop runs once per CLUSTER: the next leader is the first set bit past the previous one (a ballot over 64 words, ctz), then
//     the four waves take the later words round-robin -- lane = position -- test the set bits against the LEADER's box (compute_box_iou,
//     tube_utils.py:269-308: no "+1", every operation rounded separately, strict `>` in fp32) and clear the joiners with ONE plain 64-bit
//     store of the wave's ballot per word (a word belongs to one wave, so no atomics).  The search of the next round only reads bits past
//     the leader, the join only clears bits past it too, so ONE barrier per cluster (after the join) is enough;
//   * np.mean of a cluster's boxes is a sequential fp32 sum in list order and one division by the member count, so the sums are taken
//     one lane per cluster, the lanes of a wave walking the list together (every read is a wave-wide broadcast) and adding only their own
//     cluster's members, in order.
// Serial depth: n_clusters rounds (a barrier, a broadcast LDS read of the leader and at most ceil(n / 256) IoU tests per lane each) plus
// ceil(n_clusters / 256) walks of at most n positions -- NOT n barrier rounds (worst case n_clusters == n: no two rows overlap).  Rows past DM_LDS_ROWS are not a limit, only slower: their
// boxes and cluster numbers are read back from global memory instead of LDS.  The bitmap is sized statically: cap <= 64 * DM_WORDS rows.
#define DM_WORDS 1024
#define DM_LDS_ROWS 2048
struct DmBox { float x1, y1, x2, y2; };

__device__ __forceinline__ bool merge_iou_gt(const DmBox& a, const DmBox& b, float thr) {
    const float xmin = fmaxf(a.x1, b.x1), ymin = fmaxf(a.y1, b.y1);
    const float xmax = fminf(a.x2, b.x2), ymax = fminf(a.y2, b.y2);
    const float iw = fmaxf(__fsub_rn(xmax, xmin), 0.f), ih = fmaxf(__fsub_rn(ymax, ymin), 0.f);
    const float inter = (iw > 0.f && ih > 0.f) ? __fmul_rn(iw, ih) : 0.f;
    const float a1 = __fmul_rn(__fsub_rn(a.x2, a.x1), __fsub_rn(a.y2, a.y1));
    const float a2 = __fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1));
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(a1, a2), inter)) > thr;
}

__global__ __launch_bounds__(256) void detect_merge_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ order, const int32_t* __restrict__ sel_counts, int cap,
                                                           float thr, int32_t* cluster, int32_t* lead_pos, float* __restrict__ merged,
                                                           int32_t* __restrict__ n_clusters) {
    __shared__ unsigned long long avail[DM_WORDS];             // bit (p & 63) of word (p >> 6): position p has no cluster yet
    __shared__ __attribute__((aligned(16))) float sbox[DM_LDS_ROWS * 4];                    // the boxes of the first positions, in list order
    __shared__ int32_t scl[DM_LDS_ROWS];                       // their cluster numbers
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* B = boxes + (size_t)g * cap * 4;
    const int32_t* ord = order ? order + (size_t)g * cap : nullptr;
    int32_t* cl = cluster + (size_t)g * cap;
    int32_t* lp = lead_pos + (size_t)g * cap;
    const int n = min(max(sel_counts ? sel_counts[g] : counts[g], 0), cap);
    const int nwords = (n + 63) >> 6;

    auto row_box = [&](int p) {                                  // list position -> box, through `order` (clamped: a bad index must not leave the segment)
        const int r = ord ? min(max(ord[p], 0), cap - 1) : p;
        DmBox b = {B[4 * r], B[4 * r + 1], B[4 * r + 2], B[4 * r + 3]};
        return b;
    };
    auto box_at = [&](int p) {
        if (p < DM_LDS_ROWS) { DmBox b = {sbox[4 * p], sbox[4 * p + 1], sbox[4 * p + 2], sbox[4 * p + 3]}; return b; }
        return row_box(p);
    };

    for (int p = tid; p < min(n, DM_LDS_ROWS); p += 256) {
        const DmBox b = row_box(p);
        sbox[4 * p] = b.x1; sbox[4 * p + 1] = b.y1; sbox[4 * p + 2] = b.x2; sbox[4 * p + 3] = b.y2;
    }
    for (int w = tid; w < nwords; w += 256) avail[w] = (64 * w + 64 <= n) ? ~0ull : ((1ull << (n - 64 * w)) - 1ull);
    for (int p = n + tid; p < cap; p += 256) cl[p] = -1;
    __syncthreads();

    int K = 0;
    for (int from = 0; from < n;) {
        // next leader: the first set bit at or past `from` (every wave finds the same one)
        int L = -1;
        for (int wb = from >> 6; wb < nwords; wb += 64) {
            const int w = wb + lane;
            unsigned long long word = w < nwords ? avail[w] : 0ull;
            if (w == (from >> 6)) word &= ~0ull << (from & 63);
            const unsigned long long m = __ballot(word != 0ull);
            if (m) {
                const int src = __builtin_ctzll(m);
                const unsigned long long found = __shfl(word, src);
                L = 64 * (wb + src) + __builtin_ctzll(found);
                break;
            }
        }
        if (L < 0) break;
        const DmBox lb = box_at(L);
        const int wL = L >> 6;
        for (int w = wL + wave; w < nwords; w += 4) {
            const unsigned long long word = avail[w];
            const unsigned long long later = w == wL ? (((L & 63) == 63) ? 0ull : (~0ull << ((L & 63) + 1))) : ~0ull;
            if ((word & later) == 0ull) continue;                // wave-uniform
            const int p = 64 * w + lane;
            bool join = ((word & later) >> lane) & 1ull;
            if (join) join = merge_iou_gt(lb, box_at(p), thr);
            const unsigned long long m = __ballot(join);
            if (m) {
                if (lane == 0) avail[w] = word & ~m;
                if (join) {
                    cl[p] = K;
                    if (p < DM_LDS_ROWS) scl[p] = K;
                }
            }
        }
        if (tid == 0) {
            cl[L] = K; lp[K] = L;
            if (L < DM_LDS_ROWS) scl[L] = K;
        }
        ++K;
        from = L + 1;
        __syncthreads();
    }
    if (tid == 0) n_clusters[g] = K;

    // the means: lane = cluster, 64 consecutive clusters per wave and round; the walk starts at the first of their leaders
    for (int k0 = 64 * wave; k0 < K; k0 += 256) {
        const int k = k0 + lane;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int cnt = 0;
        int p = lp[k0];
        for (const int nl = min(n, DM_LDS_ROWS); p + 8 <= nl; p += 8) {      // eight positions' LDS reads in flight, the adds still in list order
            int c[8];
            DmBox b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { c[u] = scl[p + u]; b[u] = box_at(p + u); }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c[u] == k) {
                    s0 = __fadd_rn(s0, b[u].x1); s1 = __fadd_rn(s1, b[u].y1); s2 = __fadd_rn(s2, b[u].x2); s3 = __fadd_rn(s3, b[u].y2);
                    ++cnt;
                }
        }
        for (; p < n; ++p) {
            const int c = p < DM_LDS_ROWS ? scl[p] : cl[p];
            const DmBox b = box_at(p);
            if (c == k) {
                s0 = __fadd_rn(s0, b.x1); s1 = __fadd_rn(s1, b.y1); s2 = __fadd_rn(s2, b.x2); s3 = __fadd_rn(s3, b.y2);
                ++cnt;
            }
        }
        if (k < K) {
            float* o = merged + ((size_t)g * cap + k) * 4;
            const float d = (float)cnt;
            o[0] = __fdiv_rn(s0, d); o[1] = __fdiv_rn(s1, d); o[2] = __fdiv_rn(s2, d); o[3] = __fdiv_rn(s3, d);
        }
    }
}

// ---- frame-mAP evaluation (external/ActivityNet/Evaluation: PascalDetectionEvaluator behind utils/eval_utils.py:12-23) ------------------
// Everything here is float64, every operation rounded on its own (fp contraction is off in this file; the divisions are IEEE).

// round_sig4_kernel -- out[i] = float("{:.4}".format(in[i])): the fp32 value rounded to FOUR SIGNIFICANT decimal digits and parsed back,
// which is what the text of test.py:213 does to every box coordinate and score before the evaluator sees it.  |v| is exact in fp64; p is
// the smallest exponent with |v| * 10^p >= 1000 (the products are exact for p <= 12: a 24-bit mantissa times 5^p < 2^28 fits 53 bits, so
// the decade is found by exact comparisons, no log10); n = rint(|v| * 10^p) is the half-to-even rounding of the exact binary value that
// Python's formatting does; n / 10^p is ONE correctly rounded division of two exact doubles = the correctly rounded parse of the decimal.
// 0 -> 0 (sign kept).  |v| outside [1e-9, 1e4), inf, NaN: out = NaN and *status = 1 (a plain vector store of the same value from every
// such lane; the caller clears the word and raises when it finds it set).
__device__ const double k_pow10[13] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12};

__global__ __launch_bounds__(256) void round_sig4_kernel(const float* __restrict__ in, long long n, double* __restrict__ out,
                                                         int32_t* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = (double)in[i];
    const double a = fabs(v);
    if (a == 0.0) { out[i] = v; return; }
    double r = __builtin_nan("");
    if (a < 1e4) {                                             // (false for NaN and inf as well)
        int p = 0;
        double prod = a;
        while (prod < 1000.0 && p < 12) { ++p; prod = a * k_pow10[p]; }
        if (prod >= 1000.0) {
            double m = rint(prod);                            // 1000 .. 10000, half to even
            if (m == 10000.0) { m = 1000.0; --p; }
            r = p < 0 ? 10000.0 : m / k_pow10[p];
            if (v < 0.0) r = -r;
        }
    }
    out[i] = r;
    if (r != r) *status = 1;
}

// eval_match_kernel -- the per-image labelling (ava/per_image_evaluation.py:53-122, 388-487, 535-567), one 256-thread workgroup per IMAGE.
// The image's ground-truth rows (box, class, one claim word) sit in LDS; lanes = detection rows, in chunks of 256; a row's position in its
// image is its rank in labelling order (the caller sorted).  Pass 1: a lane walks the ground-truth rows of its class in order and keeps the
// FIRST maximum of the IoU (np.argmax; ava/np_box_ops.py:25-78) -- strict `>` -- and, where that IoU >= thresh, does
// atomicMin(&claim[gt], rank) in LDS.  One barrier.  Pass 2: true positive <=> the row's IoU passed and it holds the claim.  The reference's
// serial "walk in score order, first come first served" is exactly "lowest rank among the claimants", so there is no loop over detections.
// A row whose argmax box is taken does NOT fall back to its second-best box (neither does the reference).
// An image with more ground-truth rows than LDS holds (the host refuses them by gt_max; this is for a gt_max that understated gt_start):
// label 255 and match -2 on all its rows, uniformly for the workgroup, before any barrier.
#define EM_GT_MAX 1024
__global__ __launch_bounds__(256) void eval_match_kernel(const double* __restrict__ det_boxes, const int32_t* __restrict__ det_cls,
                                                         const long long* __restrict__ det_start, const double* __restrict__ gt_boxes,
                                                         const int32_t* __restrict__ gt_cls, const long long* __restrict__ gt_start,
                                                         double thresh, uint8_t* __restrict__ label, int32_t* __restrict__ match) {
    __shared__ double gbox[EM_GT_MAX * 4];
    __shared__ int32_t gcls[EM_GT_MAX];
    __shared__ int claim[EM_GT_MAX];
    const int k = blockIdx.x, tid = threadIdx.x;
    const long long d0 = det_start[k], g0 = gt_start[k];
    const long long nd = det_start[k + 1] - d0;
    const long long mg = gt_start[k + 1] - g0;
    if (mg > EM_GT_MAX) {                                      // the caller's gt_max was wrong: no truncated match, the image's rows say so
        for (long long r = tid; r < nd; r += 256) { label[d0 + r] = 255; match[d0 + r] = -2; }
        return;
    }
    const int m = (int)(mg < 0 ? 0 : mg);
    for (int j = tid; j < m; j += 256) {
        const double* b = gt_boxes + (g0 + j) * 4;
        gbox[4 * j] = b[0]; gbox[4 * j + 1] = b[1]; gbox[4 * j + 2] = b[2]; gbox[4 * j + 3] = b[3];
        gcls[j] = gt_cls[g0 + j];
        claim[j] = 0x7fffffff;
    }
    __syncthreads();
    for (long long r = tid; r < nd; r += 256) {
        const double* b = det_boxes + (d0 + r) * 4;
        const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        const int c = det_cls[d0 + r];
        if (!(y1 < y2 && x1 < x2)) {                           // per_image_evaluation.py:558-559 (a NaN coordinate fails it too)
            label[d0 + r] = 2; match[d0 + r] = -1;
            continue;
        }
        const double area1 = (y2 - y1) * (x2 - x1);
        int best = -1;
        double best_iou = -1.0;
        for (int j = 0; j < m; ++j) {
            if (gcls[j] != c) continue;
            const double gx1 = gbox[4 * j], gy1 = gbox[4 * j + 1], gx2 = gbox[4 * j + 2], gy2 = gbox[4 * j + 3];
            const double ih = fmax(0.0, fmin(y2, gy2) - fmax(y1, gy1));
            const double iw = fmax(0.0, fmin(x2, gx2) - fmax(x1, gx1));
            const double inter = ih * iw;
            const double area2 = (gy2 - gy1) * (gx2 - gx1);
            const double iou = inter / ((area1 + area2) - inter);
            if (iou > best_iou) { best_iou = iou; best = j; }
        }
        const bool ok = best >= 0 && best_iou >= thresh;
        if (ok) atomicMin(&claim[best], (int)r);
        match[d0 + r] = best;
        label[d0 + r] = ok ? 1 : 0;                            // (provisional: read back by this same lane behind the barrier)
    }
    __syncthreads();
    for (long long r = tid; r < nd; r += 256)
        if (label[d0 + r] == 1) label[d0 + r] = claim[match[d0 + r]] == (int)r ? 1 : 0;
}

// eval_ap_kernel -- precision, recall and average precision of one class (ava/metrics.py:22-119) on its score-descending list of labels
// (0 false / 1 true positive), one 256-thread workgroup per CLASS, the list in chunks of 256:
//   forward : ctp(i) = true positives among positions 0..i (ballot prefix in the chunk + a carried count); precision = ctp / (i + 1),
//             recall = ctp / num_gt, two rounded divisions of exact integers, as the reference's;
//   backward: chunks from the last to the first; ctp again (the carried count runs down), the precision made non-increasing from the right
//             as a suffix maximum in the chunk (shuffles in the wave, four wave maxima in LDS) + a carried maximum of the later chunks;
//             at a true positive the term (recall[i] - recall of ctp - 1) * envelope[i] -- recall changes exactly at the true positives.
// ORDER OF THE SUM (fixed, no float atomics, bit-reproducible from run to run): thread t adds its own terms -- positions t, t + 256, ... --
// starting from 0.0 in DESCENDING position order; the 256 partial sums are then added by a binary tree in LDS: stride 128, 64, ... 1,
// s[t] = s[t] + s[t + stride].  num_gt == 0: AP, precision and recall are NaN.  An empty list with ground truth: AP 0.
__global__ __launch_bounds__(256) void eval_ap_kernel(const long long* __restrict__ cls_start, const uint8_t* __restrict__ label,
                                                      const long long* __restrict__ num_gt, double* __restrict__ precision,
                                                      double* __restrict__ recall, double* __restrict__ ap) {
    __shared__ int wsum[4];
    __shared__ double wmax[4];
    __shared__ double part[256];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s0 = cls_start[c];
    const long long n = cls_start[c + 1] - s0;
    const long long ng = num_gt[c];
    if (ng <= 0) {
        const double nan = __builtin_nan("");
        for (long long i = tid; i < n; i += 256) { precision[s0 + i] = nan; recall[s0 + i] = nan; }
        if (tid == 0) ap[c] = nan;
        return;
    }
    const double dng = (double)ng;
    const long long chunks = (n + 255) / 256;
    long long carry = 0;
    for (long long ch = 0; ch < chunks; ++ch) {
        const long long i = ch * 256 + tid;
        const bool tp = i < n && label[s0 + i] == 1;
        const unsigned long long mk = __ballot(tp);
        if (lane == 0) wsum[wave] = __builtin_popcountll(mk);
        __syncthreads();
        long long ctp = carry + __builtin_popcountll(mk & ((2ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) ctp += wsum[w];
        if (i < n) {
            precision[s0 + i] = (double)ctp / (double)(i + 1);
            recall[s0 + i] = (double)ctp / dng;
        }
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    double env_later = 0.0, sum = 0.0;                         // (the reference appends a precision of 0 behind the list)
    for (long long ch = chunks - 1; ch >= 0; --ch) {
        const long long i = ch * 256 + tid;
        const bool tp = i < n && label[s0 + i] == 1;
        const unsigned long long mk = __ballot(tp);
        if (lane == 0) wsum[wave] = __builtin_popcountll(mk);
        __syncthreads();
        const long long base = carry - (wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        long long ctp = base + __builtin_popcountll(mk & ((2ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) ctp += wsum[w];
        double e = i < n ? (double)ctp / (double)(i + 1) : 0.0;
        for (int d = 1; d < 64; d <<= 1) {                     // suffix maximum inside the wave
            const double o = __shfl_down(e, d);
            if (lane + d < 64) e = fmax(e, o);
        }
        if (lane == 0) wmax[wave] = e;
        __syncthreads();
        double env = fmax(e, env_later);
        for (int w = wave + 1; w < 4; ++w) env = fmax(env, wmax[w]);
        if (tp) sum = sum + ((double)ctp / dng - (double)(ctp - 1) / dng) * env;
        env_later = fmax(env_later, fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])));
        carry = base;
        __syncthreads();
    }
    part[tid] = sum;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) part[tid] = part[tid] + part[tid + st];
        __syncthreads();
    }
    if (tid == 0) ap[c] = part[0];
}

}  // namespace step

using namespace step;

extern "C" {

int step_round_sig4(const float* in, long long n, double* out, int32_t* status, step_stream_t stream) {
    if (n < 0 || n > 0x7fffffffLL * 256) return STEP_E_SHAPE;
    if (n == 0) return STEP_OK;
    if (!in || !out || !status) return STEP_E_NULL;
    STEP_LAUNCH((round_sig4_kernel), dim3((unsigned)((n + 255) / 256)), dim3(256), stream, in, n, out, status);
    return STEP_LAUNCH_CHECK();
}

int step_eval_match(const double* det_boxes, const int32_t* det_cls, const long long* det_start, const double* gt_boxes,
                    const int32_t* gt_cls, const long long* gt_start, int NI, long long R, long long M, int gt_max, double thresh,
                    uint8_t* label, int32_t* match, step_stream_t stream) {
    if (NI < 0 || R < 0 || M < 0 || gt_max < 0 || gt_max > M) return STEP_E_SHAPE;
    if (gt_max > EM_GT_MAX) return STEP_E_UNSUPPORTED;
    if (NI == 0) return STEP_OK;
    if (!det_start || !gt_start) return STEP_E_NULL;
    if (R > 0 && (!det_boxes || !det_cls || !label || !match)) return STEP_E_NULL;
    if (M > 0 && (!gt_boxes || !gt_cls)) return STEP_E_NULL;
    if (R == 0) return STEP_OK;
    STEP_LAUNCH((eval_match_kernel), dim3((unsigned)NI), dim3(256), stream, det_boxes, det_cls, det_start, gt_boxes, gt_cls, gt_start, thresh,
                label, match);
    return STEP_LAUNCH_CHECK();
}

int step_eval_ap(const long long* cls_start, const uint8_t* label, const long long* num_gt, int NC, long long R, double* precision,
                 double* recall, double* ap, step_stream_t stream) {
    if (NC < 0 || R < 0) return STEP_E_SHAPE;
    if (NC == 0) return STEP_OK;
    if (!cls_start || !num_gt || !ap) return STEP_E_NULL;
    if (R > 0 && (!label || !precision || !recall)) return STEP_E_NULL;
    STEP_LAUNCH((eval_ap_kernel), dim3((unsigned)NC), dim3(256), stream, cls_start, label, num_gt, precision, recall, ap);
    return STEP_LAUNCH_CHECK();
}

int step_detect_merge(const float* boxes, const int32_t* counts, const int32_t* order, const int32_t* sel_counts, int G, int cap,
                      float global_thresh, int32_t* cluster, int32_t* lead_pos, float* merged, int32_t* n_clusters, step_stream_t stream) {
    if (G < 0 || cap < 0) return STEP_E_SHAPE;
    if (G == 0 || cap == 0) return STEP_OK;
    if (cap > 64 * DM_WORDS) return STEP_E_UNSUPPORTED;
    if (!boxes || !counts || !cluster || !lead_pos || !merged || !n_clusters) return STEP_E_NULL;
    if ((order == nullptr) != (sel_counts == nullptr)) return STEP_E_NULL;
    STEP_LAUNCH((detect_merge_kernel), dim3((unsigned)G), dim3(256), stream, boxes, counts, order, sel_counts, cap, global_thresh, cluster,
                lead_pos, merged, n_clusters);
    return STEP_LAUNCH_CHECK();
}

int step_detect_compact(const uint8_t* keep, const float* const* boxes, const float* const* scores, const long long* score_strides,
                        const int32_t* tube_start, int I, int B, int NC, int kmax, float width, float height, float* out_boxes,
                        float* out_scores, long long* out_cls, long long* out_tube, int32_t* counts, step_stream_t stream) {
    if (I < 0 || I > STEP_DETECT_ITERS_MAX || B < 0 || NC < 0 || kmax < 0) return STEP_E_SHAPE;
    if (I == 0 || B == 0) return STEP_OK;
    if (!counts) return STEP_E_NULL;
    const bool none = NC == 0 || kmax == 0;                    // (no flags: the launch only writes the zero counts)
    if (!none && (!keep || !boxes || !scores || !score_strides || !tube_start || !out_boxes || !out_scores || !out_cls || !out_tube)) return STEP_E_NULL;
    DetectCompactParams p;
    for (int i = 0; i < STEP_DETECT_ITERS_MAX; ++i) {
        const bool in = i < I && !none;
        p.boxes[i] = in ? boxes[i] : nullptr; p.scores[i] = in ? scores[i] : nullptr; p.score_stride[i] = in ? score_strides[i] : 0;
        if (in && (!p.boxes[i] || !p.scores[i] || p.score_stride[i] < NC)) return STEP_E_SHAPE;
    }
    p.keep = keep; p.start = tube_start; p.B = B; p.NC = NC; p.kmax = kmax; p.w = width; p.h = height;
    p.out_boxes = out_boxes; p.out_scores = out_scores; p.out_cls = out_cls; p.out_tube = out_tube; p.counts = counts;
    STEP_LAUNCH((detect_compact_kernel), dim3((unsigned)(I * B)), dim3(256), stream, p);
    return STEP_LAUNCH_CHECK();
}

size_t step_nms_scratch_bytes(int G, int kmax) {
    if (G <= 0 || kmax <= 64) return 0;
    return (size_t)G * kmax * 5 + 16;
}

int step_nms_batched(const float* boxes, const float* scores, const int32_t* counts, int G, int kmax, float threshold,
                     uint8_t* keep, void* scratch, step_stream_t stream) {
    return nms_batched_t<float>(boxes, scores, counts, G, kmax, threshold, keep, scratch, stream);
}

int step_nms_batched_f64(const double* boxes, const double* scores, const int32_t* counts, int G, int kmax, float threshold,
                         uint8_t* keep, void* scratch, step_stream_t stream) {
    return nms_batched_t<double>(boxes, scores, counts, G, kmax, threshold, keep, scratch, stream);
}

int step_detect_nms(const float* prob, long long prob_stride, int NC, const float* loc, long long loc_stride, const int32_t* tube_start,
                    const int32_t* tube_count, int B, int kmax, float conf_thresh, float nms_thresh, float width, float height,
                    uint8_t* keep, float* boxes_out, step_stream_t stream) {
    if (B < 0 || NC < 0 || kmax < 0 || prob_stride < NC || loc_stride < 4) return STEP_E_SHAPE;
    if (kmax > STEP_DETECT_TUBES_MAX) return STEP_E_UNSUPPORTED;   // (more tubes per clip: mask + step_nms_batched)
    if (B == 0 || NC == 0 || kmax == 0) return STEP_OK;
    if (!prob || !loc || !tube_start || !tube_count || !keep) return STEP_E_NULL;
    if (kmax <= 64) {
        STEP_LAUNCH((detect_nms_wave_kernel), dim3((unsigned)(B * NC)), dim3(64), stream, prob, prob_stride, NC, loc, loc_stride, tube_start,
                    tube_count, kmax, conf_thresh, nms_thresh, width, height, keep, boxes_out);
    } else {
        STEP_LAUNCH((detect_nms_block_kernel), dim3((unsigned)(B * NC)), dim3(256), stream, prob, prob_stride, NC, loc, loc_stride, tube_start,
                    tube_count, kmax, conf_thresh, nms_thresh, width, height, keep, boxes_out);
    }
    return STEP_LAUNCH_CHECK();
}

}  // extern "C"
