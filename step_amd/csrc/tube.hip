// step_amd/csrc/tube.hip -- the per-step tube bookkeeping of the multi-step inference driver as ONE launch.
//
// Replaces the host glue of utils/utils.py:68-129 (decode_coef x3 -> torch.cat -> valid_tubes -> flatten_tubes with the
// frame-index column; tube_utils.py:59-92,178-189,214-246), which the reference runs on the CPU through numpy per clip and
// which a tensor-op restatement turns into ~60 tiny element-wise launches per refinement step.  Pure fp32 element-wise
// arithmetic in the reference's operation order (no FMA contraction), one thread per (tube, output frame).
#include "common.h"

#pragma clang fp contract(off)

namespace step {

struct TubeParams {
    const float* tubes; const float* local_loc; const float* first_loc; const float* last_loc; const int32_t* clip_of;
    float* pred_loc; float* pred_first; float* pred_last; float* next_tubes;
    int N, T, Tw, first_off, last_off, extend;
    float width, height;
};

__device__ __forceinline__ void decode_box(const float* a /*x1,y1,x2,y2*/, const float* d, float (&o)[4]) {
    const float w = a[2] - a[0] + 1.0f, h = a[3] - a[1] + 1.0f;                 // get_center_size (tube_utils.py:127-134)
    const float x = a[0] + 0.5f * w, y = a[1] + 0.5f * h;
    const float px = w * d[0] + x, py = h * d[1] + y;                             // decode_coef (tube_utils.py:178-189)
    const float pw = w * expf(d[2]), ph = h * expf(d[3]);
    o[0] = px - 0.5f * pw; o[1] = py - 0.5f * ph; o[2] = px + 0.5f * pw - 1.0f; o[3] = py + 0.5f * ph - 1.0f;
}

__global__ void tube_update_kernel(TubeParams p) {
    const int Tn = p.extend ? p.T + 2 * p.Tw : p.T;
    const int Tall = p.T + 2 * p.Tw;                          // every tube decodes first | local | last (history wants all three)
    const long long total = (long long)p.N * Tall;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)blockDim.x * gridDim.x) {
        const int n = (int)(idx / Tall), u = (int)(idx % Tall);
        const float* anc; const float* del; float* dst; int tn;
        if (u < p.Tw) {                                       // first-frame neighbours: anchors = the tube's first chunk
            anc = p.tubes + ((size_t)n * p.T + p.first_off + u) * 5 + 1;
            del = p.first_loc + ((size_t)n * p.Tw + u) * 4;
            dst = p.pred_first + ((size_t)n * p.Tw + u) * 4;
            tn = p.extend ? u : -1;
        } else if (u < p.Tw + p.T) {
            const int t = u - p.Tw;
            anc = p.tubes + ((size_t)n * p.T + t) * 5 + 1;
            del = p.local_loc + ((size_t)n * p.T + t) * 4;
            dst = p.pred_loc + ((size_t)n * p.T + t) * 4;
            tn = p.extend ? u : t;
        } else {
            const int t = u - p.Tw - p.T;
            anc = p.tubes + ((size_t)n * p.T + p.last_off + t) * 5 + 1;
            del = p.last_loc + ((size_t)n * p.Tw + t) * 4;
            dst = p.pred_last + ((size_t)n * p.Tw + t) * 4;
            tn = p.extend ? u : -1;
        }
        float o[4];
        decode_box(anc, del, o);
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3];
        if (tn >= 0) {                                        // the next step's proposal: valid_tubes + the frame-index column
            float x1 = o[0] < 0.0f ? 0.0f : o[0], y1 = o[1] < 0.0f ? 0.0f : o[1];          // clamp(min = 0): NaN stays NaN
            float x2 = o[2] > p.width ? p.width : o[2], y2 = o[3] > p.height ? p.height : o[3];
            if (!((x1 < x2 - 2.0f) && (y1 < y2 - 2.0f))) { x1 = 0.0f; y1 = 0.0f; x2 = p.width; y2 = p.height; }
            float* q = p.next_tubes + ((size_t)n * Tn + tn) * 5;
            q[0] = (float)p.clip_of[n] * (float)Tn + (float)tn;
            q[1] = x1; q[2] = y1; q[3] = x2; q[4] = y2;
        }
    }
}

// ---- tube growth outside temporal_mode "predict" (step_tube_update_mode, step_tube_grow; include/step_amd.h has the contract) ----------
// "extrapolate" (tube_utils.py:159-176) and "mean" (utils.py:114-118) grow a tube from its own boxes.  A workgroup owns TB = 256 / Tn tubes
// in LDS ([tube][frame][4], Tn <= 64 frames): phase 1, a thread per (tube, frame), decodes or loads the T middle boxes; phase 2, a thread
// per (tube, side, coordinate), runs the Tw sequential steps of its side, or the mean; phase 3, a thread per (tube, output frame), clamps,
// validates or pads the box and writes its row.  One global round trip in, one out: the launch is latency-bound at tens of tubes.
__device__ __forceinline__ void valid_box(const float* b, float w, float h, float* o);     // (below, with the selection's front end)

constexpr int GROW_THREADS = 256, GROW_MAX_FRAMES = 64;
enum { GROW_EXTRAPOLATE = 1, GROW_MEAN = 2 };

struct GrowParams {
    const float* boxes; const float* local_loc; const int32_t* clip_of; const float* mask; const float* pad;
    float* pred_loc; float* out;
    int N, T, Tw, box_cols, mode, extend, validate, TB;
    float ext_x, ext_y, width, height;                        // ext_x / ext_y = ext_w - 1 / ext_h - 1: extrapolate's upper clamp
    float ca, cb;                                             // extrapolate's coefficients (grow_launch)
};

// grow(boxes[T], Tw, mode): coordinate c of one side of the tube at b (frame stride 4, Tn = T + 2 Tw frames, the middle T filled)
__device__ __forceinline__ void grow(float* b, int T, int Tw, int mode, int side, float ca, float cb) {
    const int L = T + 2 * Tw;
    if (mode == GROW_EXTRAPOLATE) {
        // every product and the difference rounded on their own (the file is compiled without contraction); sequential in i: no closed
        // form is bit-equal
        if (side) for (int i = 0; i < Tw; ++i) b[4 * (L - Tw + i)] = ca * b[4 * (L - Tw + i - 1)] - cb * b[4 * (L - 2 * Tw + i)];
        else      for (int i = 0; i < Tw; ++i) b[4 * (Tw - i - 1)] = ca * b[4 * (Tw - i)] - cb * b[4 * (2 * Tw - i - 1)];
    } else {
        float s = b[4 * Tw];                                  // np.mean(axis=1): the sequential sum in frame order / T (select_prepare_kernel's)
        for (int t = 1; t < T; ++t) s = s + b[4 * (Tw + t)];
        const float m = s / (float)T;
        const int at = side ? Tw + T : 0;
        for (int i = 0; i < Tw; ++i) b[4 * (at + i)] = m;
    }
}

__global__ __launch_bounds__(GROW_THREADS) void tube_grow_kernel(GrowParams p) {
    __shared__ float s_box[GROW_THREADS * 4];                 // TB * Tn <= 256 boxes
    const int tid = threadIdx.x;
    const int Tn = p.extend ? p.T + 2 * p.Tw : p.T, off = p.extend ? p.Tw : 0;
    const long long n0 = (long long)blockIdx.x * p.TB;
    for (int i = tid; i < p.TB * p.T; i += GROW_THREADS) {
        const int tl = i / p.T, t = i % p.T;
        const long long n = n0 + tl;
        if (n >= p.N) break;
        const size_t at = (size_t)n * p.T + t;
        float o[4];
        if (p.local_loc) {
            decode_box(p.boxes + at * 5 + 1, p.local_loc + at * 4, o);
            float* d = p.pred_loc + at * 4;
            d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3];
        } else {
            const float* q = p.boxes + at * p.box_cols + (p.box_cols - 4);
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
        }
        float* s = s_box + (tl * Tn + off + t) * 4;
        s[0] = o[0]; s[1] = o[1]; s[2] = o[2]; s[3] = o[3];
    }
    __syncthreads();
    if (p.extend) {
        for (int i = tid; i < p.TB * 8; i += GROW_THREADS) {
            const int tl = i >> 3;
            if (n0 + tl >= p.N) break;
            grow(s_box + tl * Tn * 4 + (i & 3), p.T, p.Tw, p.mode, (i >> 2) & 1, p.ca, p.cb);
        }
        __syncthreads();
    }
    for (int i = tid; i < p.TB * Tn; i += GROW_THREADS) {
        const int tl = i / Tn, t = i % Tn;
        const long long n = n0 + tl;
        if (n >= p.N) break;
        const int b = p.clip_of[n];
        float v[4];
        if (p.mask && p.mask[n] == 0.0f) {                    // a padded slot of the selection: the clip's pad, as it lies
            const float* q = p.pad + ((size_t)b * Tn + t) * 4;
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
            const float* s = s_box + i * 4;
            v[0] = s[0]; v[1] = s[1]; v[2] = s[2]; v[3] = s[3];
            if (p.extend && p.mode == GROW_EXTRAPOLATE) {     // extrapolate_tubes clamps the whole tube; np.maximum / np.minimum keep a NaN
                v[0] = v[0] < 0.0f ? 0.0f : v[0]; v[1] = v[1] < 0.0f ? 0.0f : v[1];
                v[2] = v[2] > p.ext_x ? p.ext_x : v[2]; v[3] = v[3] > p.ext_y ? p.ext_y : v[3];
            }
            if (p.validate) valid_box(v, p.width, p.height, v);
        }
        float* q = p.out + ((size_t)n * Tn + t) * 5;
        q[0] = (float)b * (float)Tn + (float)t;
        q[1] = v[0]; q[2] = v[1]; q[3] = v[2]; q[4] = v[3];
    }
}

// ---- training sample selection, device front end -------------------------------------------------------------
// What utils/utils.py:179-214 (train_select) and utils/tube_utils.py:269-351 compute per clip on the host from a previous step's
// predictions, for EVERY refined tube in one launch: the class scores averaged over the tube's frames, the three predicted tubes
// through valid_tubes, and the IoU of the tube's middle-frame box with each of its clip's ground-truth boxes.  fp32 arithmetic in
// the reference's (numpy's) operation order: the mean is the sequential sum over frames divided by T; box_iou without the +1
// convention, zero unless both overlap extents are positive; a pair with an all-zero (padding) tube gives 0.
struct SelectParams {
    const float* prob; const float* loc; const float* first; const float* last; const int32_t* clip_of; const float* gt; const int32_t* gt_count;
    float* mean_prob; float* vloc; float* vfirst; float* vlast; float* iou;
    int N, T, Tw, NC, Gmax;
    float width, height;
};

__device__ __forceinline__ void valid_box(const float* b, float w, float h, float* o) {        // tube_utils.py:59-92
    float x1 = fmaxf(0.0f, b[0]), y1 = fmaxf(0.0f, b[1]), x2 = fminf(w, b[2]), y2 = fminf(h, b[3]);
    // (np.maximum / np.minimum propagate NaN where fmaxf / fminf drop it: a NaN coordinate fails the reference's `<` test)
    const bool nan_in = (b[0] != b[0]) || (b[1] != b[1]) || (b[2] != b[2]) || (b[3] != b[3]);
    if (nan_in || !((x1 < x2 - 2.0f) && (y1 < y2 - 2.0f))) { x1 = 0.0f; y1 = 0.0f; x2 = w; y2 = h; }
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
}

__global__ void select_prepare_kernel(SelectParams p) {
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < p.NC; c += blockDim.x) {
        float s = p.prob[((size_t)n * p.T) * p.NC + c];
        for (int t = 1; t < p.T; ++t) s = s + p.prob[((size_t)n * p.T + t) * p.NC + c];
        p.mean_prob[(size_t)n * p.NC + c] = s / (float)p.T;
    }
    for (int t = threadIdx.x; t < p.T; t += blockDim.x) valid_box(p.loc + ((size_t)n * p.T + t) * 4, p.width, p.height, p.vloc + ((size_t)n * p.T + t) * 4);
    if (p.first)
        for (int t = threadIdx.x; t < p.Tw; t += blockDim.x) {
            valid_box(p.first + ((size_t)n * p.Tw + t) * 4, p.width, p.height, p.vfirst + ((size_t)n * p.Tw + t) * 4);
            valid_box(p.last + ((size_t)n * p.Tw + t) * 4, p.width, p.height, p.vlast + ((size_t)n * p.Tw + t) * 4);
        }
    const int b = p.clip_of[n];
    for (int g = threadIdx.x; g < p.Gmax; g += blockDim.x) {
        float v = 0.0f;
        if (g < p.gt_count[b]) {
            float a[4];
            valid_box(p.loc + ((size_t)n * p.T + p.T / 2) * 4, p.width, p.height, a);        // the candidate's middle frame (after valid_tubes)
            const float* q = p.gt + ((size_t)b * p.Gmax + g) * 4;
            const bool live = (((q[0] + q[1]) + q[2]) + q[3]) != 0.0f && (((a[0] + a[1]) + a[2]) + a[3]) != 0.0f;     // bool(np.sum(tube))
            if (live) {
                const float iw = fmaxf(fminf(q[2], a[2]) - fmaxf(q[0], a[0]), 0.0f);
                const float ih = fmaxf(fminf(q[3], a[3]) - fmaxf(q[1], a[1]), 0.0f);
                const float inter = (iw > 0.0f && ih > 0.0f) ? iw * ih : 0.0f;
                const float uni = (q[2] - q[0]) * (q[3] - q[1]) + (a[2] - a[0]) * (a[3] - a[1]) - inter;
                v = inter / uni;
            }
        }
        p.iou[(size_t)n * p.Gmax + g] = v;
    }
}


// ---- training sample selection, the whole rule on the device (step_select_train; include/step_amd.h has the contract) -----------------
// What train_select / select_proposals (utils/utils.py:135-423) do after the per-tube arithmetic, for one training step: one workgroup
// per clip.  The rankings, the per-candidate reductions over the ground truths, the greedy picks' scans and the output rows are spread
// over the workgroup; the shuffle and the sequential draws without replacement run on thread 0 out of LDS.  The draws come from the
// dropout generator's stream ({seed, offset} on the device), so a replayed graph selects anew on every replay.
constexpr int SEL_MAX_TUBES = 1024;                       // tubes per clip (LDS tables below)
constexpr int SEL_MAX_GT = 64;

struct SelTrainParams {
    const float* cand; const float* cfirst; const float* clast; const float* score; const float* iou; const int32_t* clip_start;
    const int32_t* clip_count;                                  // NULL: a clip owns its whole segment (step_select_train)
    const float* gt; const int32_t* gt_count; const float* pad; const unsigned long long* rng;
    float* sel; float* tgt; float* mask; int32_t* counts;
    int N, B, Tc, Tw, NC, Gmax, F, Amax, mid, before, after, topk, max_pos, neg_ratio, sampling, budget;
    float cls_thresh, reg_thresh;
};

// iou[g][tube n]: the table handed in, or (step 1) the box IoU of the tube's middle frame with ground truth g at `mid`, the arithmetic of
// select_prepare_kernel without the clamp
__device__ __forceinline__ float sel_iou(const SelTrainParams& p, int b, int g, int n) {
    if (p.iou) return p.iou[(size_t)n * p.Gmax + g];
    const float* a = p.cand + ((size_t)n * p.Tc + p.Tc / 2) * 4;
    const float* q = p.gt + (((size_t)b * p.Gmax + g) * p.F + p.mid) * (4 + p.NC);
    const bool live = (((q[0] + q[1]) + q[2]) + q[3]) != 0.0f && (((a[0] + a[1]) + a[2]) + a[3]) != 0.0f;
    if (!live) return 0.0f;
    const float iw = fmaxf(fminf(q[2], a[2]) - fmaxf(q[0], a[0]), 0.0f);
    const float ih = fmaxf(fminf(q[3], a[3]) - fmaxf(q[1], a[1]), 0.0f);
    const float inter = (iw > 0.0f && ih > 0.0f) ? iw * ih : 0.0f;
    const float uni = (q[2] - q[0]) * (q[3] - q[1]) + (a[2] - a[0]) * (a[3] - a[1]) - inter;
    return inter / uni;
}

// draw (b, phase, k): u in [0, 1) with 53 bits from words 0 and 1 of block (b << 20 | phase << 16 | k) at the state's offset
__device__ __forceinline__ double sel_draw(unsigned long long seed, unsigned long long off, int b, int phase, int k) {
    const unsigned long long blk = ((unsigned long long)b << 20) | ((unsigned long long)phase << 16) | (unsigned long long)k;
    unsigned w[4];
    philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), (unsigned)off, (unsigned)(off >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
    return (double)(((unsigned long long)w[0] << 21) | ((unsigned long long)w[1] >> 11)) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ int sel_floor(double u, int n) {               // floor(u * n), clamped to n - 1
    const int j = (int)(u * (double)n);
    return j < n - 1 ? j : n - 1;
}

enum { SEL_TAKEN = 1, SEL_ABOVE = 2, SEL_DRAWN = 4 };

__global__ __launch_bounds__(256) void select_train_kernel(SelTrainParams p) {
    __shared__ int s_cidx[SEL_MAX_TUBES];                       // candidate position -> tube of the clip
    __shared__ float s_cscore[SEL_MAX_TUBES];                   // candidate's score
    __shared__ float s_cmax[SEL_MAX_TUBES];                     // max over the ground truths of iou[g][candidate] ...
    __shared__ unsigned char s_cown[SEL_MAX_TUBES];             // ... and the first ground truth that reaches it (the owner)
    __shared__ unsigned char s_flag[SEL_MAX_TUBES];
    __shared__ float s_best[SEL_MAX_TUBES];                     // per tube: best qualifying class score
    __shared__ unsigned char s_qual[SEL_MAX_TUBES];
    __shared__ double s_w[SEL_MAX_TUBES];                       // negative-sampling weight per candidate
    __shared__ unsigned short s_rowk[SEL_MAX_TUBES];            // selected rows: candidate position, owner
    __shared__ unsigned char s_rowg[SEL_MAX_TUBES];
    __shared__ float s_rowmax[SEL_MAX_GT];
    __shared__ float s_redv[256];
    __shared__ int s_redk[256];
    __shared__ int s_n[4];                                      // candidates, positives, rows, the greedy loop's current ground truth

    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int start = p.clip_start[b];
    int A = p.clip_start[b + 1] - start;
    if (A > p.Amax) A = p.Amax;
    if (start < 0 || A < 0 || (long long)start + A > p.N) A = 0;           // (a table that does not describe [0, N): select nothing)
    if (p.clip_count) {                                                     // the segment's first clip_count[b] slots are real, the others padding
        int c = p.clip_count[b];
        c = c < 0 ? 0 : c;
        A = c < A ? c : A;
    }
    int G = p.gt_count[b];
    G = G < 0 ? 0 : G > p.Gmax ? p.Gmax : G;
    if (A == 0) G = 0;
    const int Tout = p.cfirst ? p.Tc + 2 * p.Tw : p.Tc;
    const int TW = 6 + p.NC;

    if (G > 0) {
        // ---- the candidates, in order
        if (p.score) {
            const int keep = p.topk > 0 ? 2 * (p.topk / p.NC) : A;
            for (int a = tid; a < A; a += nt) {
                bool any = false;
                float best = 0.0f;
                for (int c = 0; c < p.NC; ++c) {
                    const float s = p.score[(size_t)(start + a) * p.NC + c];
                    if (any && !(s > best)) continue;                       // cannot raise best: the class need not be ranked
                    int ahead = 0;
                    for (int o = 0; o < A && ahead < keep; ++o) {
                        const float so = p.score[(size_t)(start + o) * p.NC + c];
                        ahead += (so > s || (so == s && o < a)) ? 1 : 0;
                    }
                    if (ahead < keep) { best = s; any = true; }
                }
                s_qual[a] = any ? 1 : 0;
                s_best[a] = best;
            }
            __syncthreads();
            for (int a = tid; a < A; a += nt) {
                if (!s_qual[a]) continue;
                const float s = s_best[a];
                int rank = 0;
                for (int o = 0; o < A; ++o) rank += (s_qual[o] && (s_best[o] > s || (s_best[o] == s && o < a))) ? 1 : 0;
                if (p.topk <= 0 || rank < p.topk) { s_cidx[rank] = a; s_cscore[rank] = s; }
            }
            if (tid == 0) {
                int nq = 0;
                for (int a = 0; a < A; ++a) nq += s_qual[a];
                s_n[0] = (p.topk > 0 && nq > p.topk) ? p.topk : nq;
            }
        } else {
            for (int a = tid; a < A; a += nt) s_cidx[a] = a;
            if (tid == 0) s_n[0] = A;
        }
        __syncthreads();
        const int Ac = s_n[0];
        // ---- per candidate: maximum over the ground truths, its owner, the cls_thresh flag, the sampling weight; per ground truth: row maximum
        for (int k = tid; k < Ac; k += nt) {
            const int n = start + s_cidx[k];
            float m = sel_iou(p, b, 0, n);
            int own = 0;
            bool above = m > p.cls_thresh;
            for (int g = 1; g < G; ++g) {
                const float v = sel_iou(p, b, g, n);
                if (v > m) { m = v; own = g; }
                above = above || v > p.cls_thresh;
            }
            s_cmax[k] = m; s_cown[k] = (unsigned char)own; s_flag[k] = above ? SEL_ABOVE : 0;
            if (!p.score) s_cscore[k] = m;
            const float sc = s_cscore[k];
            s_w[k] = p.sampling == 0 ? (double)sc + 1e-6 : p.sampling == 1 ? 1.0 : exp((double)sc);
        }
        for (int g = tid; g < G; g += nt) {
            float m = sel_iou(p, b, g, start + s_cidx[0]);
            for (int k = 1; k < Ac; ++k) m = fmaxf(m, sel_iou(p, b, g, start + s_cidx[k]));
            s_rowmax[g] = m;
        }
        if (tid == 0) { s_n[1] = 0; s_n[3] = 0; }
        __syncthreads();
        // ---- first positives: G rounds, the ground truth with the largest remaining row maximum takes its best untaken candidate
        if (tid == 0) {
            int g = 0;
            for (int h = 1; h < G; ++h) if (s_rowmax[h] > s_rowmax[g]) g = h;
            s_n[3] = g;
        }
        __syncthreads();
        for (int round = 0; round < G; ++round) {
            const int g = s_n[3];
            float bv = 0.0f;
            int bk = -1;
            for (int k = tid; k < Ac; k += nt) {
                if (s_flag[k] & SEL_TAKEN) continue;
                const float v = sel_iou(p, b, g, start + s_cidx[k]);
                if (bk < 0 || v >= bv) { bv = v; bk = k; }                 // equal values: the higher candidate index
            }
            s_redv[tid] = bv; s_redk[tid] = bk;
            __syncthreads();
            if (tid == 0) {
                for (int t = 1; t < nt; ++t) {
                    const int k = s_redk[t];
                    if (k >= 0 && (bk < 0 || s_redv[t] > bv || (s_redv[t] == bv && k > bk))) { bv = s_redv[t]; bk = k; }
                }
                if (bk >= 0) {
                    s_flag[bk] |= SEL_TAKEN;
                    s_rowk[s_n[1]] = (unsigned short)bk; s_rowg[s_n[1]] = (unsigned char)g;
                    s_n[1] += 1;
                    s_rowmax[g] = -1.0f;
                }
                int ng = 0;
                for (int h = 1; h < G; ++h) if (s_rowmax[h] > s_rowmax[ng]) ng = h;
                s_n[3] = ng;
            }
            __syncthreads();
        }
        // ---- the draws: sequential by definition
        if (tid == 0) {
            const unsigned long long seed = p.rng[0], off = p.rng[1];
            int P = s_n[1];
            if (P > p.max_pos) {                                           // random.shuffle, then the first max_pos_num
                for (int i = P - 1; i >= 1; --i) {
                    const int j = sel_floor(sel_draw(seed, off, b, 0, i), i + 1);
                    const unsigned short tk = s_rowk[i]; s_rowk[i] = s_rowk[j]; s_rowk[j] = tk;
                    const unsigned char tg = s_rowg[i]; s_rowg[i] = s_rowg[j]; s_rowg[j] = tg;
                }
                P = p.max_pos;
            }
            int nab = 0;
            for (int k = 0; k < Ac; ++k) nab += (s_flag[k] & (SEL_ABOVE | SEL_TAKEN)) == SEL_ABOVE ? 1 : 0;
            if (nab > 0 && P < p.max_pos) {                                // more positives: uniform, without replacement
                const int nd = nab < p.max_pos - P ? nab : p.max_pos - P;
                for (int d = 0; d < nd; ++d) {
                    int j = sel_floor(sel_draw(seed, off, b, 1, d), nab - d);
                    int k = 0;
                    for (; k < Ac; ++k) {                                  // the j-th remaining one, ascending
                        if ((s_flag[k] & (SEL_ABOVE | SEL_TAKEN | SEL_DRAWN)) != SEL_ABOVE) continue;
                        if (j == 0) break;
                        --j;
                    }
                    if (k >= Ac) break;                                    // (cannot happen: j < the number remaining)
                    s_flag[k] |= SEL_DRAWN;
                    s_rowk[P] = (unsigned short)k; s_rowg[P] = s_cown[k];
                    ++P;
                }
            }
            int nrest = 0;
            for (int k = 0; k < Ac; ++k) {
                if (s_flag[k] & SEL_ABOVE) s_flag[k] |= SEL_TAKEN;       // never a negative: they overlap some ground truth
                s_flag[k] &= ~SEL_DRAWN;
                nrest += (s_flag[k] & SEL_TAKEN) ? 0 : 1;
            }
            int R = P;
            const long long want = (long long)P * p.neg_ratio;
            const int nneg = want < nrest ? (int)want : nrest;
            for (int d = 0; d < nneg; ++d) {                               // negatives: weighted, without replacement, sequential
                double total = 0.0;
                for (int k = 0; k < Ac; ++k) if (!(s_flag[k] & (SEL_TAKEN | SEL_DRAWN))) total += s_w[k];
                const double t = sel_draw(seed, off, b, 2, d) * total;
                double run = 0.0;
                int pick = -1;
                for (int k = 0; k < Ac; ++k) {
                    if (s_flag[k] & (SEL_TAKEN | SEL_DRAWN)) continue;
                    pick = k;
                    run += s_w[k];
                    if (run > t) break;
                }
                if (pick < 0) break;                                       // (cannot happen: nneg <= the number remaining)
                s_flag[pick] |= SEL_DRAWN;
                s_rowk[R] = (unsigned short)pick; s_rowg[R] = s_cown[pick];
                ++R;
            }
            s_n[1] = P; s_n[2] = R;
        }
    } else if (tid == 0) {
        s_n[1] = 0; s_n[2] = 0;
    }
    __syncthreads();
    const int P = s_n[1], R = s_n[2];
    if (tid == 0) { p.counts[2 * b] = P; p.counts[2 * b + 1] = R - P; }
    // ---- the clip's `budget` output rows: real rows (positives, then negatives), then the padded slots
    const size_t row0 = (size_t)b * p.budget;
    for (int r = tid; r < p.budget; r += nt) p.mask[row0 + r] = r < R ? 1.0f : 0.0f;
    for (int i = tid; i < p.budget * Tout; i += nt) {
        const int r = i / Tout, t = i % Tout;
        const float* src;
        if (r < R) {
            const size_t n = (size_t)start + s_cidx[s_rowk[r]];
            if (!p.cfirst) src = p.cand + (n * p.Tc + t) * 4;
            else if (t < p.Tw) src = p.cfirst + (n * p.Tw + t) * 4;
            else if (t < p.Tw + p.Tc) src = p.cand + (n * p.Tc + (t - p.Tw)) * 4;
            else src = p.clast + (n * p.Tw + (t - p.Tw - p.Tc)) * 4;
        } else {
            src = p.pad + ((size_t)b * Tout + t) * 4;
        }
        float* dst = p.sel + ((row0 + r) * Tout + t) * 5;
        dst[0] = (float)(b * Tout + t);
        dst[1] = src[0]; dst[2] = src[1]; dst[3] = src[2]; dst[4] = src[3];
    }
    for (int i = tid; i < p.budget * 3 * TW; i += nt) {
        const int r = i / (3 * TW), row = (i / TW) % 3, j = i % TW;
        float v = 0.0f;
        if (r < R) {
            const bool pos = r < P;
            const int frame = row == 1 ? p.mid : row == 0 ? p.before : p.after;
            const float* q = p.gt + (((size_t)b * p.Gmax + s_rowg[r]) * p.F + (frame < 0 ? 0 : frame)) * (4 + p.NC);
            if (row == 1) {
                const bool reg = pos || s_cmax[s_rowk[r]] >= p.reg_thresh;    // (a negative's owner is its arg-max ground truth)
                if (j == 4) v = pos ? 1.0f : 0.0f;
                else if (j == 5) v = reg ? 1.0f : 0.0f;
                else if (reg) v = j < 4 ? q[j] : q[j - 2];
            } else if (pos && frame >= 0) {
                if (j == 4) v = 0.0f;
                else if (j == 5) v = (((q[0] + q[1]) + q[2]) + q[3]) > 0.0f ? 1.0f : 0.0f;    // an all-zero box is padding: no regression target
                else v = j < 4 ? q[j] : q[j - 2];
            }
        }
        p.tgt[(row0 + r) * 3 * TW + i % (3 * TW)] = v;
    }
}

// behind the selection: inv = 1 / (max(real rows, 1) * NC), and the call has used its offset
__global__ __launch_bounds__(64) void select_finish_kernel(const int32_t* counts, int B, int NC, float* inv, unsigned long long* rng) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long rows = 0;
    for (int b = 0; b < B; ++b) rows += (long long)counts[2 * b] + counts[2 * b + 1];
    if (rows < 1) rows = 1;
    inv[0] = (float)(1.0 / (double)(rows * NC));
    rng[1] += 1ull;
}

// ---- classification pre-training: boxes sampled around the ground truths (step_anchor_sample; include/step_amd.h has the rule) --------
// What data/ava_cls.py:200-261 (sample_anchors) does per ground-truth box inside the loader's __getitem__ -- up to 100 sequential trials,
// each a jaccard_numpy call -- for all clips of a batch in one launch.  A trial's outcome does not depend on earlier trials, only which
// accepted trials are TAKEN does: one wave per (clip, ground truth) pair, lane = trial (50 of 64), two ballots per loop, and the "up to the
// pos_num-th positive" / "the first n negatives" rules are bit operations on the ballot masks.  One workgroup walks the pairs, a wave each
// per round, so that the rows can be written compactly behind an exclusive prefix of the per-pair row counts.  float64 throughout, every
// operation rounded on its own (the file is compiled without contraction), draws from the generator's stream like select_train_kernel.
constexpr int ANC_TRIALS = 50;
constexpr int ANC_MAX_WAVES = 16;

struct AnchorParams {
    const float* gt; const int32_t* gt_count; unsigned long long* rng;
    float* tubes; int32_t* clip_start; int32_t* counts;
    int B, Gmax, F, NC, mid, T, pos_num, neg_num, mode;
    double W, H, pos_thresh, neg_thresh;
};

__device__ __forceinline__ double anc_min(double a, double b) { return b < a ? b : a; }           // Python's min(a, b) / max(a, b): the first
__device__ __forceinline__ double anc_max(double a, double b) { return b > a ? b : a; }           // argument unless the second one beats it
__device__ __forceinline__ double anc_uniform(double a, double b, double u) { return a + (b - a) * u; }   // random.uniform

// the box of ground truth g of clip b at frame `mid`, divided by (W, H, W, H)
__device__ __forceinline__ void anc_box(const AnchorParams& p, int b, int g, double (&a)[4]) {
    const float* q = p.gt + (((size_t)b * p.Gmax + g) * p.F + p.mid) * (4 + p.NC);
    a[0] = (double)q[0] / p.W; a[1] = (double)q[1] / p.H; a[2] = (double)q[2] / p.W; a[3] = (double)q[3] / p.H;
}

// jaccard_numpy(anchors, c) against the G boxes of the clip: bit 0 = P (own IoU above pos_thresh, every other one below neg_thresh),
// bit 1 = N (all G below neg_thresh)
__device__ __forceinline__ int anc_accept(const AnchorParams& p, int b, int g, int G, const double (&c)[4]) {
    const double area_c = (c[2] - c[0]) * (c[3] - c[1]);
    int below = 0;
    bool own = false;
    for (int o = 0; o < G; ++o) {
        double a[4];
        anc_box(p, b, o, a);
        double iw = (a[2] < c[2] ? a[2] : c[2]) - (a[0] > c[0] ? a[0] : c[0]);
        double ih = (a[3] < c[3] ? a[3] : c[3]) - (a[1] > c[1] ? a[1] : c[1]);
        iw = iw < 0.0 ? 0.0 : iw; ih = ih < 0.0 ? 0.0 : ih;
        const double inter = iw * ih;
        const double uni = (a[2] - a[0]) * (a[3] - a[1]) + area_c - inter;
        const double iou = inter / uni;
        below += iou < p.neg_thresh ? 1 : 0;
        if (o == g) own = iou > p.pos_thresh;
    }
    return ((own && below == G - 1) ? 1 : 0) | (below == G ? 2 : 0);
}

__device__ __forceinline__ unsigned long long anc_first(unsigned long long m, int n) {            // the lowest n set bits of m
    unsigned long long r = 0;
    for (int i = 0; i < n && m; ++i) { r |= m & (~m + 1ull); m &= m - 1ull; }
    return r;
}

__global__ __launch_bounds__(64 * ANC_MAX_WAVES) void anchor_sample_kernel(AnchorParams p) {
    __shared__ int s_rows[ANC_MAX_WAVES];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const unsigned long long seed = p.rng[0], off = p.rng[1];
    const int npairs = p.B * p.Gmax;
    const int S = p.pos_num + p.neg_num;
    const size_t rowlen = (size_t)p.T * 4;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int base = 0; base < npairs; base += nw) {
        const int q = base + wave;
        const int b = q < npairs ? q / p.Gmax : 0, g = q < npairs ? q % p.Gmax : 0;
        int G = 0;
        if (q < npairs) { G = p.gt_count[b]; G = G < 0 ? 0 : G > p.Gmax ? p.Gmax : G; }
        const bool live = q < npairs && g < G;
        double ca[4] = {0.0, 0.0, 0.0, 0.0}, cb[4] = {0.0, 0.0, 0.0, 0.0};
        unsigned long long posm = 0, nega = 0, negb = 0;
        int npos = 0;
        if (live) {                                                        // (wave-uniform: all 64 lanes take part in the ballots)
            double a[4];
            anc_box(p, b, g, a);
            const double w = a[2] - a[0], h = a[3] - a[1];
            const double x = a[0] + 0.5 * w, y = a[1] + 0.5 * h;
            const bool trial = lane < ANC_TRIALS;
            const int j = trial ? lane : 0;
            if (p.mode == 0) {                                             // loop A (ava_cls.py:216-232)
                const double nwd = anc_uniform(0.8 * w, anc_min(1.0, 1.2 * w), sel_draw(seed, off, q, 0, 16 * j + 0));
                const double nhd = anc_uniform(0.8 * h, anc_min(1.0, 1.2 * h), sel_draw(seed, off, q, 0, 16 * j + 1));
                const double nx = anc_uniform(anc_max(0.5 * nwd, x - 0.2 * w), anc_min(1.0 - 0.5 * nwd, x + 0.2 * w), sel_draw(seed, off, q, 0, 16 * j + 2));
                const double ny = anc_uniform(anc_max(0.5 * nhd, y - 0.2 * h), anc_min(1.0 - 0.5 * nhd, y + 0.2 * h), sel_draw(seed, off, q, 0, 16 * j + 3));
                ca[0] = nx - 0.5 * nwd; ca[1] = ny - 0.5 * nhd; ca[2] = nx + 0.5 * nwd; ca[3] = ny + 0.5 * nhd;
                const int acc = anc_accept(p, b, g, G, ca);
                const unsigned long long Pm = __ballot(trial && (acc & 1)), Nm = __ballot(trial && (acc & 2));
                unsigned long long m = Pm;                                 // j*: the trial of the pos_num-th P, or the last trial
                int seen = m ? 1 : 0;
                for (; seen < p.pos_num && (m & (m - 1ull)); ++seen) m &= m - 1ull;
                const int jstar = (seen == p.pos_num) ? __builtin_ctzll(m) : ANC_TRIALS - 1;
                const unsigned long long upto = (2ull << jstar) - 1ull;
                posm = Pm & upto;
                nega = anc_first(Nm & upto, p.neg_num);
                npos = __builtin_popcountll(posm);
            } else {
                npos = 1;                                                  // eval: the ground-truth box itself
            }
            {                                                              // loop B (ava_cls.py:236-252)
                double u[12];
                for (int k = 0; k < 12; ++k) u[k] = sel_draw(seed, off, q, 1, 16 * j + k);
                const double w0 = anc_uniform(0.3 * w, 0.7 * w, u[0]), w1 = anc_min(1.0, anc_uniform(1.5 * w, 2.0 * w, u[1]));
                const double nwd = u[2] < 0.5 ? w0 : w1;
                const double h0 = anc_uniform(0.3 * h, 0.7 * h, u[3]), h1 = anc_min(1.0, anc_uniform(1.5 * h, 2.0 * h, u[4]));
                const double nhd = u[5] < 0.5 ? h0 : h1;
                const double x0 = anc_uniform(anc_max(0.5 * nwd, x - w), anc_max(0.5 * nwd, x - 0.3 * w), u[6]);
                const double x1 = anc_uniform(anc_min(1.0 - 0.5 * nwd, x + 0.3 * w), anc_min(1.0 - 0.5 * nwd, x + w), u[7]);
                const double nx = u[8] < 0.5 ? x0 : x1;
                const double y0 = anc_uniform(anc_max(0.5 * nhd, x - h), anc_max(0.5 * nhd, y - 0.3 * h), u[9]);       // x - h: the reference's line 242
                const double y1 = anc_uniform(anc_min(1.0 - 0.5 * nhd, y + 0.3 * h), anc_min(1.0 - 0.5 * nhd, y + h), u[10]);
                const double ny = u[11] < 0.5 ? y0 : y1;
                cb[0] = nx - 0.5 * nwd; cb[1] = ny - 0.5 * nhd; cb[2] = nx + 0.5 * nwd; cb[3] = ny + 0.5 * nhd;
                const int acc = anc_accept(p, b, g, G, cb);
                const unsigned long long Nm = __ballot(trial && (acc & 2));
                negb = anc_first(Nm, p.neg_num - __builtin_popcountll(nega));
            }
        }
        const int na = __builtin_popcountll(nega), nneg = na + __builtin_popcountll(negb);
        const int prow = live ? (npos > 0 ? npos : 1) : 0;                 // no positive: the ground-truth box stands in
        if (lane == 0) s_rows[wave] = prow + nneg;
        __syncthreads();
        int row0 = s_base, total = 0;
        for (int v = 0; v < nw; ++v) { if (v < wave) row0 += s_rows[v]; total += s_rows[v]; }
        if (q < npairs && lane == 0) {
            p.counts[2 * q] = npos; p.counts[2 * q + 1] = nneg;
            if (g == 0) p.clip_start[b] = row0;
        }
        if (live) {
            const unsigned long long below = (1ull << lane) - 1ull;
            const double sc[4] = {p.W, p.H, p.W, p.H};
            int r = -1;
            float v4[4];
            if (posm >> lane & 1ull) {
                r = __builtin_popcountll(posm & below);
                for (int k = 0; k < 4; ++k) v4[k] = (float)(ca[k] * sc[k]);
            } else if (nega >> lane & 1ull) {
                r = prow + __builtin_popcountll(nega & below);
                for (int k = 0; k < 4; ++k) v4[k] = (float)(ca[k] * sc[k]);
            }
            if (r >= 0) {
                float* dst = p.tubes + ((size_t)row0 + r) * rowlen;
                for (int t = 0; t < p.T; ++t) { dst[4 * t] = v4[0]; dst[4 * t + 1] = v4[1]; dst[4 * t + 2] = v4[2]; dst[4 * t + 3] = v4[3]; }
            }
            if (negb >> lane & 1ull) {                                     // (a lane can hold a row of loop A and one of loop B)
                r = prow + na + __builtin_popcountll(negb & below);
                float* dst = p.tubes + ((size_t)row0 + r) * rowlen;
                for (int k = 0; k < 4; ++k) v4[k] = (float)(cb[k] * sc[k]);
                for (int t = 0; t < p.T; ++t) { dst[4 * t] = v4[0]; dst[4 * t + 1] = v4[1]; dst[4 * t + 2] = v4[2]; dst[4 * t + 3] = v4[3]; }
            }
            if (npos == 0 || p.mode != 0) {                                // the box itself, bit for bit
                const float* src = p.gt + (((size_t)b * p.Gmax + g) * p.F + p.mid) * (4 + p.NC);
                float* dst = p.tubes + (size_t)row0 * rowlen;
                for (int i = lane; i < p.T * 4; i += 64) dst[i] = src[i & 3];
            }
        }
        __syncthreads();
        if (tid == 0) s_base += total;                                     // (read again only behind the next round's barrier)
    }
    __syncthreads();
    const int rows = s_base;
    if (tid == 0) { p.clip_start[p.B] = rows; p.rng[1] = off + 1ull; }
    if (npairs == 0) for (int b = tid; b < p.B; b += blockDim.x) p.clip_start[b] = 0;
    const size_t end = (size_t)npairs * S * rowlen;
    for (size_t i = (size_t)rows * rowlen + tid; i < end; i += blockDim.x) p.tubes[i] = 0.0f;
}

// ---- the augmentation's decisions on the device (step_augment_plan; include/step_amd.h has the rule) ---------------------------------------
// What TubeAugmentation.plan (step_amd/augment.py) draws per clip on the host: one wavefront per clip writes the clip's step_aug_clip, its
// erase rectangles and the transformed ground truths.  A trial of the crop or of get_region depends on its own draws only, so the 50 (64)
// trials of a round are evaluated with lane = trial and the first accepted one is taken by ballot: the sequential rule's result.  The tubes
// are never stored: every stage after the crop is element-wise given (rectangle, kept set, mirror), so a box is recomputed where it is used.
constexpr int AUGP_CROP_ROUNDS = 16, AUGP_CROP_TRIALS = 50, AUGP_ERASE_TRIALS = 64, AUGP_MODE_K = AUGP_CROP_ROUNDS * AUGP_CROP_TRIALS * 4;

struct AugPlanParams {
    const unsigned long long* src; const int32_t* dims; const float* gt_in; const int32_t* gt_count; const unsigned long long* rng;
    unsigned char* block; float* gt_out; int32_t* gt_count_out;
    int N, Gmax, F, NC, switches, scale, Wn, Hn, cap_words;
    const float* tubes_in; const int32_t* tube_count; const float* fill; float* tubes_out; int32_t* tube_count_out;      // step_augment_plan_tubes
    int Pmax, Tp, n_fill;
};

__device__ __forceinline__ float augp_div(float a, float b) { return (float)((double)a / (double)b); }     // IEEE fp32 quotient and root, whatever
__device__ __forceinline__ float augp_sqrt(float a) { return (float)sqrt((double)a); }                    // the build's fast-math settings

struct AugpState { int W, H, cropped, r0, r1, r2, r3, mirror, width, height; };

// box (g, f) of clip n in pixels of the cropped, mirrored frame: _scale_xy, _shift_into + the clamp at 0, the mirror
__device__ __forceinline__ void augp_box(const AugPlanParams& p, const AugpState& s, int n, int g, int f, float (&b)[4]) {
    const float* q = p.gt_in + (((size_t)n * p.Gmax + g) * p.F + f) * (4 + p.NC);
    b[0] = q[0] * (float)s.W; b[1] = q[1] * (float)s.H; b[2] = q[2] * (float)s.W; b[3] = q[3] * (float)s.H;
    if (s.cropped) {
        const float x0 = (float)s.r0, y0 = (float)s.r1, x1 = (float)s.r2, y1 = (float)s.r3;
        b[0] = fmaxf((b[0] > x0 ? b[0] : x0) - x0, 0.0f);
        b[1] = fmaxf((b[1] > y0 ? b[1] : y0) - y0, 0.0f);
        b[2] = fmaxf((b[2] < x1 ? b[2] : x1) - x0, 0.0f);
        b[3] = fmaxf((b[3] < y1 ? b[3] : y1) - y0, 0.0f);
    }
    if (s.mirror && (((b[0] + b[1]) + b[2]) + b[3]) > 0.0f) {                 // (zero-padded boxes stay where they are)
        const float l = (float)s.width - b[2], r = (float)s.width - b[0];
        b[0] = l; b[2] = r;
    }
}

__global__ __launch_bounds__(64) void augment_plan_kernel(AugPlanParams p) {
    __shared__ int s_rect[4];
    __shared__ int s_fits;
    const int n = blockIdx.x, lane = threadIdx.x;
    const unsigned long long seed = p.rng[0], off = p.rng[1];
    int32_t* words = (int32_t*)p.block;
    const int rect_base = 16 * p.N + 6 * p.Gmax * n;
    const int rec_at = 16 * p.N + 6 * p.Gmax * p.N;                           // the call record, then the patches
    const int patch_base = rec_at + 4;
    AugpState s;
    s.H = p.dims[2 * n]; s.W = p.dims[2 * n + 1];
    s.H = s.H < 1 ? 1 : s.H; s.W = s.W < 1 ? 1 : s.W;
    s.cropped = 0; s.r0 = 0; s.r1 = 0; s.r2 = s.W; s.r3 = s.H; s.mirror = 0; s.width = s.W; s.height = s.H;
    int G = p.gt_count[n];
    G = G < 0 ? 0 : G > p.Gmax ? p.Gmax : G;
    const int mid = p.F / 2;

    // photometric coins and parameters: phase 0, one fixed slot per draw of the host rule
    int flags = 0, perm = 0x24;
    float par[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.switches & STEP_AUGP_PHOTOMETRIC) {
        flags |= STEP_AUG_PHOTOMETRIC;
        if (sel_floor(sel_draw(seed, off, n, 0, 0), 2)) { flags |= STEP_AUG_BRIGHTNESS; par[0] = (float)anc_uniform(-32.0, 32.0, sel_draw(seed, off, n, 0, 1)); }
        const int first = sel_floor(sel_draw(seed, off, n, 0, 2), 2);
        if (first) {
            flags |= STEP_AUG_CONTRAST_FIRST;
            if (sel_floor(sel_draw(seed, off, n, 0, 3), 2)) { flags |= STEP_AUG_CONTRAST; par[1] = (float)anc_uniform(0.5, 1.5, sel_draw(seed, off, n, 0, 4)); }
        }
        if (sel_floor(sel_draw(seed, off, n, 0, 5), 2)) { flags |= STEP_AUG_SATURATION; par[2] = (float)anc_uniform(0.5, 1.5, sel_draw(seed, off, n, 0, 6)); }
        if (sel_floor(sel_draw(seed, off, n, 0, 7), 2)) { flags |= STEP_AUG_HUE; par[3] = (float)anc_uniform(-18.0, 18.0, sel_draw(seed, off, n, 0, 8)); }
        if (!first && sel_floor(sel_draw(seed, off, n, 0, 9), 2)) { flags |= STEP_AUG_CONTRAST; par[1] = (float)anc_uniform(0.5, 1.5, sel_draw(seed, off, n, 0, 10)); }
        if (sel_floor(sel_draw(seed, off, n, 0, 11), 2)) {
            const int k = sel_floor(sel_draw(seed, off, n, 0, 12), 6);        // _PERMS[k], packed 2 bits per channel
            perm = k == 0 ? 0x24 : k == 1 ? 0x18 : k == 2 ? 0x21 : k == 3 ? 0x09 : k == 4 ? 0x12 : 0x06;
        }
    }

    // RandomSampleCrop: phase 1
    unsigned long long keep = G >= 64 ? ~0ull : (1ull << G) - 1ull;
    double crop_w = 0.0, crop_h = 0.0;                                        // the accepted trial's drawn sizes: valid_tubes' window for the proposals
    if (p.switches & STEP_AUGP_CROP) {
        const double Wd = (double)s.W, Hd = (double)s.H;
        for (int round = 0; round < AUGP_CROP_ROUNDS; ++round) {
            const int mode = sel_floor(sel_draw(seed, off, n, 1, AUGP_MODE_K + round), 7);
            if (mode == 0) break;                                             // None: the whole frame
            const double thr = mode == 1 ? 0.1 : mode == 2 ? 0.3 : mode == 3 ? 0.5 : mode == 4 ? 0.7 : mode == 5 ? 0.9 : -INFINITY;
            const bool trial = lane < AUGP_CROP_TRIALS;
            const int kb = (round * AUGP_CROP_TRIALS + (trial ? lane : 0)) * 4;
            const double w = anc_uniform(0.3 * Wd, Wd, sel_draw(seed, off, n, 1, kb + 0));
            const double h = anc_uniform(0.3 * Hd, Hd, sel_draw(seed, off, n, 1, kb + 1));
            bool ok = trial && !(h / w < 0.5 || h / w > 2.0);
            int r[4] = {0, 0, 0, 0};
            unsigned long long kept = 0;
            if (ok) {
                const double lw = Wd - w, lh = Hd - h;
                const double left = lw + (1.0 - lw) * sel_draw(seed, off, n, 1, kb + 2);
                const double top = lh + (1.0 - lh) * sel_draw(seed, off, n, 1, kb + 3);
                r[0] = (int)left; r[1] = (int)top; r[2] = (int)(left + w); r[3] = (int)(top + h);
                // (a rectangle that is empty or leaves the frame is no crop: step_clip_augment_u8 trusts the block)
                ok = r[0] >= 0 && r[1] >= 0 && r[2] > r[0] && r[3] > r[1] && r[2] <= s.W && r[3] <= s.H;
            }
            if (ok) {
                const double area_r = (double)((long long)(r[2] - r[0]) * (long long)(r[3] - r[1]));
                double m = INFINITY;
                bool nan = false;
                for (int g = 0; g < G; ++g) {
                    float b[4];
                    augp_box(p, s, n, g, mid, b);                             // (s is still the uncropped, unmirrored state)
                    const double hx = (double)b[2] < (double)r[2] ? (double)b[2] : (double)r[2], hy = (double)b[3] < (double)r[3] ? (double)b[3] : (double)r[3];
                    const double lx = (double)b[0] > (double)r[0] ? (double)b[0] : (double)r[0], ly = (double)b[1] > (double)r[1] ? (double)b[1] : (double)r[1];
                    double sx = hx - lx, sy = hy - ly;
                    sx = sx < 0.0 ? 0.0 : sx; sy = sy < 0.0 ? 0.0 : sy;
                    const double inter = sx * sy;
                    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
                    const double ov = inter / (((double)area_b + area_r) - inter);
                    if (ov != ov) nan = true;
                    m = ov < m ? ov : m;
                    const float cx = (b[0] + b[2]) / 2.0f, cy = (b[1] + b[3]) / 2.0f;
                    if ((double)r[0] < (double)cx && (double)r[1] < (double)cy && (double)r[2] > (double)cx && (double)r[3] > (double)cy) kept |= 1ull << g;
                }
                if (!nan && m < thr) ok = false;                              // (numpy's min() hands a NaN on, and NaN < x is false)
                if (kept == 0) ok = false;
            }
            const unsigned long long acc = __ballot(ok);
            if (acc) {
                const int win = __builtin_ctzll(acc);
                if (lane == win) { s_rect[0] = r[0]; s_rect[1] = r[1]; s_rect[2] = r[2]; s_rect[3] = r[3]; }
                keep = __shfl(kept, win);
                crop_w = __shfl(w, win); crop_h = __shfl(h, win);
                __syncthreads();
                s.cropped = 1; s.r0 = s_rect[0]; s.r1 = s_rect[1]; s.r2 = s_rect[2]; s.r3 = s_rect[3];
                s.width = s.r2 - s.r0; s.height = s.r3 - s.r1;
                break;
            }
        }
    }
    const int K = __builtin_popcountll(keep);

    // mirror and the erase coin: phase 2
    if ((p.switches & STEP_AUGP_FLIP) && sel_floor(sel_draw(seed, off, n, 2, 0), 2)) { s.mirror = 1; flags |= STEP_AUG_MIRROR; }
    const bool erase = (p.switches & STEP_AUGP_ERASE) && sel_floor(sel_draw(seed, off, n, 2, 1), 2);

    // the proposals (step_augment_plan_tubes): a clip owns Pmax slots, the first `cnt` real -- its own, transformed in double on the fp32
    // inputs as TubeAugmentation.plan does with float64 proposals, or the fill rows when it has none -- the others the whole frame
    if (p.tubes_out) {
        int P = p.tube_count[n];
        P = P < 0 ? 0 : P > p.Pmax ? p.Pmax : P;
        const bool filled = P == 0 && p.fill;
        const int cnt = filled ? (p.n_fill < p.Pmax ? p.n_fill : p.Pmax) : P;
        const size_t base = (size_t)n * p.Pmax * p.Tp;
        for (int i = lane; i < p.Pmax * p.Tp; i += 64) {
            const int j = i / p.Tp;
            double b[4] = {0.0, 0.0, 1.0, 1.0};
            if (j < cnt) {
                if (filled) {                                                 // (the reference builds the anchors behind the transform)
                    const float* q = p.fill + (size_t)j * 4;
                    b[0] = (double)q[0]; b[1] = (double)q[1]; b[2] = (double)q[2]; b[3] = (double)q[3];
                } else {
                    const float* q = p.tubes_in + (base + i) * 4;
                    b[0] = (double)q[0] * (double)s.W; b[1] = (double)q[1] * (double)s.H; b[2] = (double)q[2] * (double)s.W; b[3] = (double)q[3] * (double)s.H;
                    if (s.cropped) {                                          // _shift_into, then valid_tubes(width = w, height = h)
                        const double x0 = (double)s.r0, y0 = (double)s.r1, x1 = (double)s.r2, y1 = (double)s.r3;
                        b[0] = anc_max(b[0], x0) - x0; b[1] = anc_max(b[1], y0) - y0;
                        b[2] = anc_min(b[2], x1) - x0; b[3] = anc_min(b[3], y1) - y0;
                        b[0] = anc_max(b[0], 0.0); b[1] = anc_max(b[1], 0.0); b[2] = anc_min(b[2], crop_w); b[3] = anc_min(b[3], crop_h);
                        if (!(b[0] < b[2] - 2.0 && b[1] < b[3] - 2.0)) { b[0] = 0.0; b[1] = 0.0; b[2] = crop_w; b[3] = crop_h; }
                    }
                    if (s.mirror) {                                           // (every box: no zero-box exemption for proposals)
                        const double l = (double)s.width - b[2], r = (double)s.width - b[0];
                        b[0] = l; b[2] = r;
                    }
                    b[0] = b[0] / (double)s.width; b[1] = b[1] / (double)s.height; b[2] = b[2] / (double)s.width; b[3] = b[3] / (double)s.height;
                }
                for (int c = 0; c < 4; ++c) b[c] = anc_min(anc_max(b[c], 0.0), 1.0);
            }
            float* o = p.tubes_out + (base + i) * 4;
            o[0] = (float)(b[0] * (double)p.Wn); o[1] = (float)(b[1] * (double)p.Hn); o[2] = (float)(b[2] * (double)p.Wn); o[3] = (float)(b[3] * (double)p.Hn);
        }
        if (lane == 0) p.tube_count_out[n] = cnt;
    }

    // RandomErase.get_region per kept box, in order: phase 3
    int n_rects = 0;
    if (erase) {
        unsigned long long rest = keep;
        for (int j = 0; j < K; ++j) {
            const int g = __builtin_ctzll(rest);
            rest &= rest - 1ull;
            float b[4];
            augp_box(p, s, n, g, mid, b);
            const float S = (b[2] - b[0]) * (b[3] - b[1]);
            const int kb = (j * AUGP_ERASE_TRIALS + lane) * 4;
            const float Se = (float)anc_uniform(0.02, 0.2, sel_draw(seed, off, n, 3, kb + 0)) * S;
            const float re = (float)anc_uniform(0.3, 10.0 / 3.0, sel_draw(seed, off, n, 3, kb + 1));
            const float He = augp_sqrt(Se * re), We = augp_sqrt(augp_div(Se, re));
            const double xe = anc_uniform((double)b[0], (double)(b[2] - We), sel_draw(seed, off, n, 3, kb + 2));
            const double ye = anc_uniform((double)b[1], (double)(b[3] - He), sel_draw(seed, off, n, 3, kb + 3));
            const float xr = (float)xe + We, yr = (float)ye + He;
            const bool ok = xr <= b[2] && yr <= b[3];
            const unsigned long long acc = __ballot(ok);
            if (!acc) continue;                                               // 64 trials rejected: nothing erased for this box
            const int win = __builtin_ctzll(acc);
            if (lane == win) {
                const int x1 = (int)xe, y1 = (int)ye, x2 = (int)xr, y2 = (int)yr;
                // a rectangle outside its crop or larger than a patch slot is dropped (the bound of the header rules the second out)
                const bool fits = x1 >= 0 && y1 >= 0 && x1 <= x2 && y1 <= y2 && x2 <= s.width && y2 <= s.height &&
                                  (long long)(x2 - x1) * (long long)(y2 - y1) * 3 <= (long long)p.cap_words;
                s_fits = fits; s_rect[0] = x1; s_rect[1] = y1; s_rect[2] = x2; s_rect[3] = y2;
            }
            __syncthreads();
            const int fits = s_fits, x1 = s_rect[0], y1 = s_rect[1], x2 = s_rect[2], y2 = s_rect[3];
            __syncthreads();
            if (!fits) continue;
            if (lane == 0) {
                int32_t* rc = words + rect_base + 6 * n_rects;
                rc[0] = x1; rc[1] = y1; rc[2] = x2; rc[3] = y2;
                rc[4] = patch_base + (n * p.Gmax + n_rects) * p.cap_words; rc[5] = 0;
            }
            ++n_rects;
        }
    }
    for (int i = 6 * n_rects + lane; i < 6 * p.Gmax; i += 64) words[rect_base + i] = 0;

    if (lane == 0) {
        int32_t* c = words + 16 * n;
        *(unsigned long long*)c = p.src[n];
        c[2] = s.H; c[3] = s.W; c[4] = s.r0; c[5] = s.r1; c[6] = s.width; c[7] = s.height; c[8] = flags; c[9] = perm;
        float* cf = (float*)c;
        cf[10] = par[0]; cf[11] = par[1]; cf[12] = par[2]; cf[13] = par[3];
        c[14] = n_rects; c[15] = rect_base;
        p.gt_count_out[n] = K;
        if (n == 0) { words[rec_at] = (int32_t)(unsigned)off; words[rec_at + 1] = (int32_t)(unsigned)(off >> 32); words[rec_at + 2] = 0; words[rec_at + 3] = 0; }
    }

    // the ground truths the loader hands on: kept tubes compacted in index order, percent of the crop, scale_tubes_abs to (Wn, Hn)
    const int E = 4 + p.NC, per = p.F * E;
    float* out = p.gt_out + (size_t)n * p.Gmax * per;
    for (int i = lane; i < p.Gmax * per; i += 64) {
        const int j = i / per, f = (i % per) / E, c = i % E;
        float v = 0.0f;
        if (j < K) {
            unsigned long long m = keep;
            for (int t = 0; t < j; ++t) m &= m - 1ull;
            const int g = __builtin_ctzll(m);
            if (c >= 4) {
                v = p.gt_in[(((size_t)n * p.Gmax + g) * p.F + f) * E + c];
            } else {
                float b[4];
                augp_box(p, s, n, g, f, b);
                const float bc = c == 0 ? b[0] : c == 1 ? b[1] : c == 2 ? b[2] : b[3];
                const float pc = augp_div(bc, (float)((c & 1) ? s.height : s.width));
                const float cl = fminf(fmaxf(pc, 0.0f), 1.0f);
                v = cl * (float)((c & 1) ? p.Hn : p.Wn);
            }
        }
        out[i] = v;
    }
}

// the erase patches of the rectangles the planner accepted: element e of patch (n, k) is word e & 3 of block ((n Gmax + k) << 20) | (e >> 2)
// at the planner's offset + 1, which every thread takes from the call record in the block; thread (0, 0) advances the generator by the call's
// 2 (the planner has finished, and nothing here reads the state's offset)
constexpr int AUGP_NOISE_RUN = 8;                                             // Philox blocks per thread
__global__ __launch_bounds__(64) void augment_noise_kernel(unsigned char* block, int N, int Gmax, int cap_words, double lo, double hi,
                                                           unsigned long long* rng) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) rng[1] += 2ull;
    if (N * Gmax == 0) return;
    const int32_t* words = (const int32_t*)block;
    const int slot = blockIdx.y, n = slot / Gmax, k = slot % Gmax;
    if (k >= words[16 * n + 14]) return;
    const int rec_at = 16 * N + 6 * Gmax * N;
    const int32_t* rc = words + 16 * N + 6 * Gmax * n + 6 * k;
    long long used = (long long)(rc[2] - rc[0]) * (rc[3] - rc[1]) * 3;
    used = used < cap_words ? used : cap_words;                                // (the planner dropped what would not fit: belt and braces)
    const unsigned long long seed = rng[0];
    const unsigned long long off = (((unsigned long long)(unsigned)words[rec_at + 1] << 32) | (unsigned long long)(unsigned)words[rec_at]) + 1ull;
    float* dst = (float*)block + rc[4];
    for (int i = 0; i < AUGP_NOISE_RUN; ++i) {
        const long long q = ((long long)blockIdx.x * AUGP_NOISE_RUN + i) * 64 + threadIdx.x, e0 = 4 * q;
        if (e0 >= used) return;
        const unsigned long long blk = ((unsigned long long)slot << 20) | (unsigned long long)q;
        unsigned w[4];
        philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), (unsigned)off, (unsigned)(off >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
        const float v0 = (float)(lo + (hi - lo) * ((double)(w[0] >> 8) * (1.0 / 16777216.0))), v1 = (float)(lo + (hi - lo) * ((double)(w[1] >> 8) * (1.0 / 16777216.0)));
        const float v2 = (float)(lo + (hi - lo) * ((double)(w[2] >> 8) * (1.0 / 16777216.0))), v3 = (float)(lo + (hi - lo) * ((double)(w[3] >> 8) * (1.0 / 16777216.0)));
        dst[e0] = v0;
        if (e0 + 1 < used) dst[e0 + 1] = v1;
        if (e0 + 2 < used) dst[e0 + 2] = v2;
        if (e0 + 3 < used) dst[e0 + 3] = v3;
    }
}

}  // namespace step

using namespace step;

// the patch slot of step_augment_plan in words: 3 * (floor(0.2 A + 2 sqrt(2 A / 3) + 1) + 2), A = the largest Hs * Ws (header: derivation)
static long long augp_cap_words(long long max_hw) {
    const double A = (double)max_hw;
    return 3 * ((long long)(0.2 * A + 2.0 * sqrt(2.0 * A / 3.0) + 1.0) + 2);
}

extern "C" size_t step_augment_plan_bytes(int N, int Gmax, long long max_hw, int* cap_words) {
    if (N < 0 || Gmax < 0 || max_hw < 1) return 0;
    const long long cap = augp_cap_words(max_hw);
    if (cap_words) *cap_words = cap > 0x7fffffffLL ? 0 : (int)cap;
    const long long words = 16ll * N + 6ll * Gmax * N + 4 + (long long)N * Gmax * cap;
    return (size_t)(4 * ((words + 3) / 4 * 4));
}

extern "C" int step_augment_plan_tubes(const unsigned long long* src, const int32_t* dims, const float* gt_in, const int32_t* gt_count, int N, int Gmax,
                                       int F, int NC, int switches, int scale, int Wn, int Hn, long long max_hw, unsigned long long* rng_state,
                                       void* plan_block, float* gt_out, int32_t* gt_count_out, const float* tubes_in, const int32_t* tube_count,
                                       int Pmax, int Tp, const float* fill, int n_fill, float* tubes_out, int32_t* tube_count_out,
                                       step_stream_t stream) {
    if (N < 0 || Gmax < 0 || F <= 0 || NC < 0 || Wn < 1 || Hn < 1 || max_hw < 1) return STEP_E_SHAPE;
    if (scale < 0 || scale > 2 || (switches & ~15)) return STEP_E_SHAPE;
    if (tubes_in && (Pmax < 0 || Tp < 1 || n_fill < 0)) return STEP_E_SHAPE;
    if (Gmax > SEL_MAX_GT || (tubes_in && Pmax > SEL_MAX_TUBES)) return STEP_E_UNSUPPORTED;
    if (tubes_in && (long long)N * Pmax * Tp > 0x1fffffffLL) return STEP_E_UNSUPPORTED;
    const long long cap = augp_cap_words(max_hw);
    if (cap > (1ll << 22)) return STEP_E_UNSUPPORTED;                          // (a patch's elements are addressed by 20 bits of Philox block)
    if (16ll * N + 6ll * Gmax * N + 4 + (long long)N * Gmax * cap > 0x7fffffffLL || (long long)N * Gmax > 65535) return STEP_E_UNSUPPORTED;
    if (!rng_state) return STEP_E_NULL;
    if ((uintptr_t)rng_state & 7) return STEP_E_ALIGN;
    if (tubes_in && (!tube_count || !tubes_out || !tube_count_out)) return STEP_E_NULL;
    if (N > 0) {
        if (!src || !dims || !gt_count || !plan_block || !gt_count_out || (Gmax && (!gt_in || !gt_out))) return STEP_E_NULL;
        if ((uintptr_t)plan_block & 15) return STEP_E_ALIGN;
        AugPlanParams p;
        p.src = src; p.dims = dims; p.gt_in = gt_in; p.gt_count = gt_count; p.rng = rng_state;
        p.block = (unsigned char*)plan_block; p.gt_out = gt_out; p.gt_count_out = gt_count_out;
        p.N = N; p.Gmax = Gmax; p.F = F; p.NC = NC; p.switches = switches; p.scale = scale; p.Wn = Wn; p.Hn = Hn; p.cap_words = (int)cap;
        p.tubes_in = tubes_in; p.tube_count = tube_count; p.fill = n_fill > 0 ? fill : nullptr; p.tubes_out = tubes_in ? tubes_out : nullptr;
        p.tube_count_out = tube_count_out; p.Pmax = Pmax; p.Tp = Tp; p.n_fill = n_fill;
        STEP_LAUNCH(augment_plan_kernel, dim3((unsigned)N), dim3(64), stream, p);
    }
    const double lo = scale == 2 ? -1.0 : 0.0, hi = scale == 0 ? 255.0 : 1.0;
    const long long slots = (long long)N * Gmax;
    const unsigned gx = slots > 0 ? (unsigned)((cap + 4 * 64 * AUGP_NOISE_RUN - 1) / (4 * 64 * AUGP_NOISE_RUN)) : 1u;
    STEP_LAUNCH(augment_noise_kernel, dim3(gx, (unsigned)(slots > 0 ? slots : 1)), dim3(64), stream, (unsigned char*)plan_block, N, Gmax,
                (int)cap, lo, hi, rng_state);                                  // (also for N == 0: the call counts)
    return STEP_LAUNCH_CHECK();
}

extern "C" int step_augment_plan(const unsigned long long* src, const int32_t* dims, const float* gt_in, const int32_t* gt_count, int N, int Gmax,
                                 int F, int NC, int switches, int scale, int Wn, int Hn, long long max_hw, unsigned long long* rng_state,
                                 void* plan_block, float* gt_out, int32_t* gt_count_out, step_stream_t stream) {
    return step_augment_plan_tubes(src, dims, gt_in, gt_count, N, Gmax, F, NC, switches, scale, Wn, Hn, max_hw, rng_state, plan_block, gt_out,
                                   gt_count_out, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int step_anchor_sample(const float* gt, const int32_t* gt_count, int B, int Gmax, int F, int NC, int mid, float width, float height,
                                  int T, int pos_num, int neg_ratio, float pos_thresh, float neg_thresh, int mode, unsigned long long* rng_state,
                                  float* tubes, int32_t* clip_start, int32_t* counts, step_stream_t stream) {
    if (B < 0 || Gmax < 0 || F <= 0 || NC < 0 || mid < 0 || mid >= F || (mode != 0 && mode != 1)) return STEP_E_SHAPE;
    if (pos_num < 1 || neg_ratio < 0 || T < 1) return STEP_E_SHAPE;
    const long long S = (long long)pos_num * (1 + (long long)neg_ratio);
    if (Gmax > SEL_MAX_GT || (long long)Gmax * S > SEL_MAX_TUBES) return STEP_E_UNSUPPORTED;
    if ((long long)B * Gmax > 0x3fffffffLL) return STEP_E_UNSUPPORTED;
    if (!rng_state || !clip_start) return STEP_E_NULL;
    if ((uintptr_t)rng_state & 7) return STEP_E_ALIGN;
    const long long npairs = (long long)B * Gmax;
    if (npairs > 0 && (!gt || !gt_count || !tubes || !counts)) return STEP_E_NULL;
    AnchorParams p;
    p.gt = gt; p.gt_count = gt_count; p.rng = rng_state; p.tubes = tubes; p.clip_start = clip_start; p.counts = counts;
    p.B = B; p.Gmax = Gmax; p.F = F; p.NC = NC; p.mid = mid; p.T = T; p.pos_num = pos_num; p.neg_num = npairs > 0 ? pos_num * neg_ratio : 0; p.mode = mode;
    p.W = (double)width; p.H = (double)height; p.pos_thresh = (double)pos_thresh; p.neg_thresh = (double)neg_thresh;
    const int waves = npairs < 1 ? 1 : npairs > ANC_MAX_WAVES ? ANC_MAX_WAVES : (int)npairs;
    STEP_LAUNCH(anchor_sample_kernel, dim3(1), dim3(64u * (unsigned)waves), stream, p);
    return STEP_LAUNCH_CHECK();
}

extern "C" int step_select_prepare(const float* prob, const float* loc, const float* first, const float* last, int N, int T, int Tw, int NC,
                                   const int32_t* clip_of, const float* gt_mid, const int32_t* gt_count, int Gmax, float width, float height,
                                   float* mean_prob, float* vloc, float* vfirst, float* vlast, float* iou, step_stream_t stream) {
    if (N < 0 || T <= 0 || NC <= 0 || Gmax < 0 || Tw < 0) return STEP_E_SHAPE;
    if (N == 0) return STEP_OK;
    if (!prob || !loc || !clip_of || !mean_prob || !vloc || (Gmax && (!gt_mid || !gt_count || !iou))) return STEP_E_NULL;
    if ((first != nullptr) != (last != nullptr) || (first && (!vfirst || !vlast || Tw <= 0))) return STEP_E_NULL;
    SelectParams p;
    p.prob = prob; p.loc = loc; p.first = first; p.last = last; p.clip_of = clip_of; p.gt = gt_mid; p.gt_count = gt_count;
    p.mean_prob = mean_prob; p.vloc = vloc; p.vfirst = vfirst; p.vlast = vlast; p.iou = iou;
    p.N = N; p.T = T; p.Tw = Tw; p.NC = NC; p.Gmax = Gmax; p.width = width; p.height = height;
    STEP_LAUNCH(select_prepare_kernel, dim3((unsigned)N), dim3(64), stream, p);
    return STEP_LAUNCH_CHECK();
}

extern "C" int step_select_train_counted(const float* cand, const float* cand_first, const float* cand_last, const float* score, const float* iou,
                                         int N, int Tc, int Tw, int NC, const int32_t* clip_start, int B, int Amax, const float* gt,
                                         const int32_t* gt_count, int Gmax, int F, const float* pad_tubes, unsigned long long* rng_state, int mid,
                                         int before, int after, int topk, float cls_thresh, float reg_thresh, int max_pos_num, int neg_ratio,
                                         int sampling, int budget, float* sel, float* tgt, float* mask, float* inv, int32_t* counts,
                                         const int32_t* clip_count, step_stream_t stream) {
    if (N < 0 || B < 0 || Tc <= 0 || Tw < 0 || NC <= 0 || Gmax < 0 || F <= 0 || Amax < 0 || budget <= 0) return STEP_E_SHAPE;
    if (mid < 0 || mid >= F || (before < 0) != (after < 0) || before >= F || after >= F) return STEP_E_SHAPE;
    if (max_pos_num < 0 || neg_ratio < 0 || sampling < 0 || sampling > 2) return STEP_E_SHAPE;
    if ((long long)budget < (long long)max_pos_num * (1 + (long long)neg_ratio)) return STEP_E_SHAPE;      // the slots can then never overflow
    if (topk > 0 && topk < NC) return STEP_E_SHAPE;
    if (Amax > SEL_MAX_TUBES || Gmax > SEL_MAX_GT) return STEP_E_UNSUPPORTED;
    if ((long long)B * budget * (Tc + 2 * Tw > 3 * (6 + NC) ? Tc + 2 * Tw : 3 * (6 + NC)) > 0x7fffffffLL) return STEP_E_UNSUPPORTED;
    if (!rng_state || !inv || (B > 0 && !counts)) return STEP_E_NULL;
    if ((uintptr_t)rng_state & 7) return STEP_E_ALIGN;
    if (B > 0) {
        if (!clip_start || !gt_count || !pad_tubes || !sel || !tgt || !mask || (Gmax && !gt) || (N > 0 && !cand)) return STEP_E_NULL;
        if ((cand_first != nullptr) != (cand_last != nullptr) || (cand_first && Tw <= 0)) return STEP_E_NULL;
        SelTrainParams p;
        p.cand = cand; p.cfirst = cand_first; p.clast = cand_last; p.score = score; p.iou = iou; p.clip_start = clip_start;
        p.gt = gt; p.gt_count = gt_count; p.pad = pad_tubes; p.rng = rng_state; p.clip_count = clip_count;
        p.sel = sel; p.tgt = tgt; p.mask = mask; p.counts = counts;
        p.N = N; p.B = B; p.Tc = Tc; p.Tw = Tw; p.NC = NC; p.Gmax = Gmax; p.F = F; p.Amax = Amax; p.mid = mid; p.before = before; p.after = after;
        p.topk = topk; p.max_pos = max_pos_num; p.neg_ratio = neg_ratio; p.sampling = sampling; p.budget = budget;
        p.cls_thresh = cls_thresh; p.reg_thresh = reg_thresh;
        const int threads = Amax <= 64 ? 64 : Amax <= 128 ? 128 : 256;
        STEP_LAUNCH(select_train_kernel, dim3((unsigned)B), dim3((unsigned)threads), stream, p);
    }
    STEP_LAUNCH(select_finish_kernel, dim3(1), dim3(64), stream, (const int32_t*)counts, B, NC, inv, rng_state);      // (also for B == 0: the call counts)
    return STEP_LAUNCH_CHECK();
}

extern "C" int step_select_train(const float* cand, const float* cand_first, const float* cand_last, const float* score, const float* iou,
                                 int N, int Tc, int Tw, int NC, const int32_t* clip_start, int B, int Amax, const float* gt,
                                 const int32_t* gt_count, int Gmax, int F, const float* pad_tubes, unsigned long long* rng_state, int mid,
                                 int before, int after, int topk, float cls_thresh, float reg_thresh, int max_pos_num, int neg_ratio,
                                 int sampling, int budget, float* sel, float* tgt, float* mask, float* inv, int32_t* counts,
                                 step_stream_t stream) {
    return step_select_train_counted(cand, cand_first, cand_last, score, iou, N, Tc, Tw, NC, clip_start, B, Amax, gt, gt_count, Gmax, F, pad_tubes,
                                     rng_state, mid, before, after, topk, cls_thresh, reg_thresh, max_pos_num, neg_ratio, sampling, budget, sel, tgt,
                                     mask, inv, counts, nullptr, stream);
}

extern "C" int step_tube_update(const float* tubes, int N, int T, const float* local_loc, const float* first_loc, const float* last_loc,
                                int Tw, int first_off, int last_off, const int32_t* clip_of, int extend, float width, float height,
                                float* pred_loc, float* pred_first, float* pred_last, float* next_tubes, step_stream_t stream) {
    if (N < 0 || T <= 0 || Tw <= 0 || first_off < 0 || last_off < 0 || first_off + Tw > T || last_off + Tw > T) return STEP_E_SHAPE;
    if (N == 0) return STEP_OK;
    if (!tubes || !local_loc || !first_loc || !last_loc || !clip_of || !pred_loc || !pred_first || !pred_last || !next_tubes) return STEP_E_NULL;
    TubeParams p;
    p.tubes = tubes; p.local_loc = local_loc; p.first_loc = first_loc; p.last_loc = last_loc; p.clip_of = clip_of;
    p.pred_loc = pred_loc; p.pred_first = pred_first; p.pred_last = pred_last; p.next_tubes = next_tubes;
    p.N = N; p.T = T; p.Tw = Tw; p.first_off = first_off; p.last_off = last_off; p.extend = extend ? 1 : 0;
    p.width = width; p.height = height;
    const long long total = (long long)N * (T + 2 * Tw);
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    STEP_LAUNCH(tube_update_kernel, dim3((unsigned)g), dim3(256), stream, p);
    return STEP_LAUNCH_CHECK();
}

// the checks step_tube_update_mode and step_tube_grow share: the growth's own limits
static int grow_check(int T, int Tw, int mode, int extend) {
    if (mode != GROW_EXTRAPOLATE && mode != GROW_MEAN) return STEP_E_SHAPE;
    if (extend && mode == GROW_EXTRAPOLATE && (Tw < 2 || T < Tw)) return STEP_E_SHAPE;      // (division by Tw - 1; the recurrence reaches Tw frames back)
    if ((extend ? T + 2 * Tw : T) > GROW_MAX_FRAMES) return STEP_E_UNSUPPORTED;
    return STEP_OK;
}

static int grow_launch(GrowParams& p, float ext_w, float ext_h, step_stream_t stream) {
    const int Tn = p.extend ? p.T + 2 * p.Tw : p.T;
    p.TB = GROW_THREADS / Tn;
    p.ext_x = ext_w - 1.0f; p.ext_y = ext_h - 1.0f;
    // the reference's Python-float coefficients T / (T - 1) and 1 / (T - 1), rounded to fp32 once where numpy multiplies an fp32 array by them
    p.ca = p.Tw > 1 ? (float)((double)p.Tw / (double)(p.Tw - 1)) : 0.0f; p.cb = p.Tw > 1 ? (float)(1.0 / (double)(p.Tw - 1)) : 0.0f;
    const long long g = ((long long)p.N + p.TB - 1) / p.TB;
    STEP_LAUNCH(tube_grow_kernel, dim3((unsigned)g), dim3(GROW_THREADS), stream, p);
    return STEP_LAUNCH_CHECK();
}

extern "C" int step_tube_update_mode(const float* tubes, int N, int T, const float* local_loc, const int32_t* clip_of, int mode, int extend,
                                     int Tw, float ext_w, float ext_h, float width, float height, float* pred_loc, float* next_tubes,
                                     step_stream_t stream) {
    if (N < 0 || T <= 0 || Tw <= 0) return STEP_E_SHAPE;
    const int rc = grow_check(T, Tw, mode, extend ? 1 : 0);
    if (rc != STEP_OK) return rc;
    if (N == 0) return STEP_OK;
    if (!tubes || !local_loc || !clip_of || !pred_loc || !next_tubes) return STEP_E_NULL;
    GrowParams p;
    p.boxes = tubes; p.local_loc = local_loc; p.clip_of = clip_of; p.mask = nullptr; p.pad = nullptr; p.pred_loc = pred_loc; p.out = next_tubes;
    p.N = N; p.T = T; p.Tw = Tw; p.box_cols = 5; p.mode = mode; p.extend = extend ? 1 : 0; p.validate = 1;
    p.width = width; p.height = height;
    return grow_launch(p, ext_w, ext_h, stream);
}

extern "C" int step_tube_grow(const float* boxes, int box_cols, int N, int T, int Tw, int mode, float ext_w, float ext_h, const int32_t* clip_of,
                              const float* mask, const float* pad_tubes, int validate, float width, float height, float* out,
                              step_stream_t stream) {
    if (N < 0 || T <= 0 || Tw <= 0 || (box_cols != 4 && box_cols != 5) || (validate != 0 && validate != 1)) return STEP_E_SHAPE;
    const int rc = grow_check(T, Tw, mode, 1);
    if (rc != STEP_OK) return rc;
    if (N == 0) return STEP_OK;
    if (!boxes || !clip_of || !out || (mask != nullptr) != (pad_tubes != nullptr)) return STEP_E_NULL;
    GrowParams p;
    p.boxes = boxes; p.local_loc = nullptr; p.clip_of = clip_of; p.mask = mask; p.pad = pad_tubes; p.pred_loc = nullptr; p.out = out;
    p.N = N; p.T = T; p.Tw = Tw; p.box_cols = box_cols; p.mode = mode; p.extend = 1; p.validate = validate;
    p.width = width; p.height = height;
    return grow_launch(p, ext_w, ext_h, stream);
}
