// step_amd/csrc/conv_tap_narrow.h -- the PIXEL-SPLIT form of the two-phase 3x3x3 conv for the narrow members of a grouped launch
// (step_conv_forward_group: an Inception block's branch_2 conv, Cin <= 32 -> Cout <= 96, beside its wide branch_1 partner), and the
// grouped kernels that carry it.  Included by conv_tap_ph_{bf16,f16}.hip.
#pragma once
#include "conv_tap_kernel.h"

namespace step {

// Why a second body.  Inside conv_tap_body a narrow member takes the instantiation of its wide partner (NB = the partner's depth), whose two
// wave groups are the two CHANNEL halves of a 256-pixel x 64*NB-channel tile:
//   * 96 channels at NB = 3 (Mixed_3c) fill group 0 only; group 1 keeps the barriers and does nothing, so the anti-phase scheme has no
//     partner and every step's load phase and multiply phase run one after the other on half of the CU's waves;
//   * 32 channels at NB = 2 (Mixed_3b): group 0 also multiplies its second block against a clamped duplicate of block 0;
//   * Cin = 16 / 24 is zero-padded to the 32-channel slab: at Cin = 16 the second k16 step of every tap multiplies zeros;
//   * 256-pixel tiles give a K loop of 14 steps per ~9 us of prologue + epilogue + drain.
// Here the eight waves split the PIXEL axis: every wave owns 64 pixels x ALL NBn = ceil(Cout / 32) channel blocks (acc[2][NBn], at most 96
// accumulator registers), the two wave groups (waves w and w + 4 share a SIMD) are the two pixel halves of a 512-pixel box and run the L / C
// phases in anti-phase exactly as conv_tap_body's two-phase form does.  Both groups read the SAME weights: one ring of two step buffers, staged
// once per step by all 512 threads -- each thread writes its share of step s + 1 during its OWN L phase of step s; group 1 runs half a step
// (one phase) behind group 0, so buffer (s + 1) & 1 is written in phases 2s (group 0) and 2s + 1 (group 1), after its last readers (step
// s - 1: phases 2s - 2 and 2s - 1) and before its first (step s + 1: phase 2s + 2).
//   * KS = 1 when Cin <= 16: only the first k16 block of a pixel is staged and multiplied.  The halo keeps conv_tap_body's 80-byte pixel
//     pitch: the fragment reads are the j = 0 reads of that layout, conflict-free by the argument at conv_tap_kernel.h (HWPAD / gmode), and
//     the 512-pixel halo (at most NARROW_NPIX pixels: 6 x 6 x 30 = 1080 for the 4 x 4 x 28 box of the 28-wide maps) still fits: 90 KiB.
//   * TPS = taps per barrier pair, chosen so that a C phase is 12-24 MFMAs per wave whatever NBn * KS: 9 taps (three steps) at one block x one
//     k16 step, 3 taps (nine steps) in between, 2 taps (fourteen steps; the zero tap that pads 27 to 28 is neither read nor multiplied) at
//     NBn * KS = 6.  The tap order stays 0 .. 26 and k16 steps ascend inside a tap: per output the same products in the same order into one
//     fp32 accumulator, the same affine + ReLU + rounding -- bit-identical to step_conv_forward.  (The all-zero k16 step and the duplicate
//     block that are dropped change no bit: fp32 acc + (+-0) is acc, and accumulators start at +0.)
//   * Weights come from the ordinary packed image ([block][tap padded][KC16][fragment]); one slab, so the whole K loop is unrolled.
constexpr int NARROW_NPIX = CONV_NARROW_NPIX;               // halo pixels reserved for a 512-pixel box
constexpr int NARROW_BSTEP_MAX = 12 * 1024;                 // weight bytes of one step: TPS * NBn * KS fragments <= 12
constexpr int NARROW_LDS_BYTES = NARROW_NPIX * 80 + 2 * NARROW_BSTEP_MAX + 3 * 32 * 2 * 4;
__host__ __device__ constexpr int narrow_tps(int nbn, int ks) { return nbn * ks == 1 ? 9 : (nbn * ks >= 6 ? 2 : 3); }

template <typename T, int NBn, int KS>
__device__ __forceinline__ void conv_tap_narrow_body(const ConvParams& p, unsigned char* lds) {
    static_assert(sizeof(T) == 2 && NBn >= 1 && NBn <= 3 && (KS == 1 || KS == 2), "16-bit storage, one slab, at most three channel blocks");
    constexpr int NT = 512, MB = 2, ES = 2, VEC = 8, PITCH = 80, SLOTS = 2 * KS;
    constexpr int KH = 3, KW = 3, NTAPS = 27, NTP = taps_padded(NTAPS);
    constexpr int TPS = narrow_tps(NBn, KS);
    constexpr int SPS = (NTAPS + TPS - 1) / TPS;           // steps of the K loop: 3, 9 or 14
    constexpr int FRAGB = 512 * ES, FRAGV = FRAGB / 16;
    constexpr int HB = NBn * KS * FRAGB;                    // bytes of one tap's weights
    constexpr int BSTEP = TPS * HB, BVEC = BSTEP / 16, Q = (BVEC + NT - 1) / NT;
    static_assert(BSTEP <= NARROW_BSTEP_MAX && SPS >= 3, "ring buffer size; the prologue issues three steps");
    constexpr int ITER = (NARROW_NPIX * SLOTS + NT - 1) / NT;
    typedef u16x8 vec16;
    typedef typename frag<T>::type frag_t;
    const int TD = p.gtd, TH = p.gth, TW = p.gtw;
    const int TPX = TD * TH * TW;                           // <= 512
    const int HH_ = TH + KH - 1, HW_ = TW + KW - 1, PD = TD + 2;
    const int HHW = HH_ * HW_, NPIX = PD * HHW, NVEC = NPIX * SLOTS;
    unsigned char* const ldsA = lds;
    unsigned char* const ldsB = lds + NARROW_NPIX * PITCH;
    float* const ldsS = (float*)(ldsB + 2 * NARROW_BSTEP_MAX);

    // accumulator row m (0 .. 511) -> box coordinates: conv_tap_body's general-box maps with sixteen 32-row blocks (p.gmode = 1: every
    // 16-lane service group of a ds_read_b128 takes 16 consecutive columns of one box row; 0: linear walk, rows past the box alias pixel 0)
    auto tile_pix = [&](int m, int& td, int& th, int& tw) -> bool {
        if (p.gmode) {
            const int pl_ = m & 31, blk = m >> 5;
            int g, j;
            if (pl_ < 4) { g = 0; j = pl_; }
            else if (pl_ < 12) { g = 1; j = pl_ - 4; }
            else if (pl_ < 16) { g = 0; j = pl_ - 8; }
            else if (pl_ < 20) { g = 1; j = pl_ - 8; }
            else if (pl_ < 28) { g = 0; j = pl_ - 12; }
            else { g = 1; j = pl_ - 16; }
            const int spr = (TW + 15) >> 4;
            const int slot = blk * 2 + g;
            const int row = slot / spr, col = (slot % spr) * 16 + j;
            const bool ok = row < TD * TH && col < TW;
            const int rc = row < TD * TH ? row : 0;
            tw = col; th = rc % TH; td = rc / TH;
            return ok;
        }
        const int mc = m < TPX ? m : 0;
        tw = mc % TW; const int q = mc / TW; th = q % TH; td = q / TH;
        return m < TPX;
    };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
#ifdef STEP_EMUL
    const int wave = tid >> 6;
#else
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
    const int khalf = lane >> 5;
    const int grp = wave >> 2;                              // wave group = pixel half (waves w and w + 4 share a SIMD)
    const int m0 = grp * 256 + (wave & 3) * (MB * 32);      // this wave's first accumulator row

    int gbx, gby;
    if (!grid_coords(p, gbx, gby)) return;                  // (padding ids of the remapped grid: before any barrier)
    int t = gbx + p.tile0;
    const int tw_i = t % p.tiles_w; t /= p.tiles_w;
    const int th_i = t % p.tiles_h; t /= p.tiles_h;
    const int d0 = (t % p.tiles_d) * TD, n = t / p.tiles_d;
    const int h0 = th_i * TH, w0 = tw_i * TW;
    const int KC16 = p.nchunks32 * 2;

    const T* xg = (const T*)p.x;
    const unsigned char* wg = (const unsigned char*)p.w;

    // ---- weights: all 512 threads stage the ONE ring; a step's tile is [tap][block][k16][fragment] in LDS
    const unsigned char* wthr[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int v = min(tid + q * NT, BVEC - 1);         // (threads past the tile re-load its last vector and do not store it)
        const int tp = v / (HB / 16), rem = v % (HB / 16);
        const int f = rem / FRAGV, within = rem % FRAGV;
        const int nbl = f / KS, ks = f % KS;
        wthr[q] = wg + (((size_t)nbl * NTP + tp) * KC16 + ks) * FRAGB + within * 16;
    }
    const unsigned wstep = (unsigned)TPS * KC16 * FRAGB;   // bytes between consecutive steps
    auto load_B = [&](int si, u32x4 (&r)[Q]) {
#pragma unroll
        for (int q = 0; q < Q; ++q) r[q] = *(const u32x4*)(wthr[q] + (size_t)((unsigned)si * wstep));
    };
    auto store_B = [&](int bufoff, const u32x4 (&r)[Q]) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if ((q + 1) * NT <= BVEC || tid + q * NT < BVEC) *(u32x4*)(ldsB + bufoff + (tid + q * NT) * 16) = r[q];
    };
    u32x4 R0[Q], R1[Q];                                    // weights in flight: R0 even steps, R1 odd steps
    load_B(0, R0);
    load_B(1, R1);
#ifndef STEP_EMUL
    __builtin_amdgcn_sched_barrier(0);                     // (the halo's index arithmetic runs under the weights' latency, as in conv_tap_body)
#endif
    float ss_sc = 1.f, ss_sh = 0.f;
    if (tid < NBn * 32) {
        const int co = min(tid, p.Cout - 1);
        if (p.scale) ss_sc = p.scale[co];
        if (p.shift) ss_sh = p.shift[co];
    }
    // ---- halo: SLOTS 16-byte vectors per pixel (KS = 1: channels 0 .. 15 only), zeros outside the image and past Cin
    {
        unsigned goff[ITER];
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int v = tid + it * NT;
            goff[it] = ~0u;
            if (v < NVEC) {
                const int pix = v / SLOTS, slot = v % SLOTS;
                const int plane = (int)__umulhi((unsigned)pix, p.mag_hhw), rem = pix - plane * HHW;
                const int r = (int)__umulhi((unsigned)rem, p.mag_hw), cc = rem - r * HW_;
                const int id = d0 + plane - 1, ih = h0 + r - 1, iw = w0 + cc - 1;
                if (id >= 0 && id < p.D && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W && slot * VEC < p.Cin) {
                    const size_t gpix = (((size_t)n * p.D + id) * p.H + ih) * p.W + iw;
                    goff[it] = (unsigned)(gpix * p.x_cstride + p.x_coff + slot * VEC);
                }
            }
        }
        vec16 stage[ITER];
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            vec16 val;
#pragma unroll
            for (int e = 0; e < VEC; ++e) val[e] = 0;
            if (goff[it] != ~0u) val = *(const vec16*)(xg + (size_t)goff[it]);
            stage[it] = val;
        }
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int v = tid + it * NT;
            if (v < NVEC) *(vec16*)(ldsA + (v / SLOTS) * PITCH + ((v % SLOTS) << 4)) = stage[it];
        }
    }
    if (tid < NBn * 32) { ldsS[tid] = ss_sc; ldsS[NBn * 32 + tid] = ss_sh; }
    store_B(0, R0);
    load_B(2, R0);

    // LDS byte offsets of this lane's two accumulator rows (before the tap shift), incl. its k half
    int aoff[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        int td_, th_, tw_;
        tile_pix(m0 + mb * 32 + (lane & 31), td_, th_, tw_);
        aoff[mb] = ((td_ * HH_ + th_) * HW_ + tw_) * PITCH + khalf * 16;
    }
    f32x16 acc[MB][NBn];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < NBn; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][i][r] = 0.f;
    __syncthreads();

    frag_t fa[TPS][KS][MB], fb[TPS][KS][NBn];
    const unsigned char* const bwave = ldsB + lane * (8 * ES);
    const int HHWB = HHW * PITCH, HWB = HW_ * PITCH;
    // step s: fragments from ring buffer s & 1; the register set of the other parity holds step s + 1, is written to ring buffer (s + 1) & 1
    // and re-issued for step s + 3
    auto step = [&](auto sic) {
        constexpr int SI = decltype(sic)::value;
        constexpr int QP = SI & 1;
        u32x4 (&Rn)[Q] = QP ? R0 : R1;
        // ---- L: all of the step's fragments LDS -> registers, then the weight hand-over
#pragma unroll
        for (int tp = 0; tp < TPS; ++tp) {
            const int tap = SI * TPS + tp;                 // (compile-time after unrolling)
            if (tap >= NTAPS) continue;                    // the zero tap that pads 27 to 28
            int shift = (tap / (KH * KW)) * HHWB + ((tap / KW) % KH) * HWB + (tap % KW) * PITCH;
#ifndef STEP_EMUL
            asm volatile("" : "+s"(shift));                // run-time box: pin the shift to this phase (see conv_tap_body)
#endif
#pragma unroll
            for (int j = 0; j < KS; ++j) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) fa[tp][j][mb] = lds_read_bfrag<T>(lds + aoff[mb] + shift + j * 32);
#pragma unroll
                for (int i = 0; i < NBn; ++i) fb[tp][j][i] = lds_read_bfrag<T>(bwave + QP * BSTEP + tp * HB + (i * KS + j) * FRAGB);
            }
        }
        if constexpr (SI + 1 < SPS) store_B((QP ^ 1) * BSTEP, Rn);
#ifndef STEP_EMUL
        __builtin_amdgcn_sched_barrier(0);                 // the weight requests go BEHIND the fragment reads
#endif
        if constexpr (SI + 3 < SPS) load_B(SI + 3, Rn);
#ifndef STEP_EMUL
        __builtin_amdgcn_sched_barrier(0);
#endif
        __syncthreads();
        // ---- C: the step's MFMAs back to back out of registers, at raised priority (the partner wave is in its L phase)
#ifndef STEP_EMUL
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
        for (int tp = 0; tp < TPS; ++tp) {
            if (SI * TPS + tp >= NTAPS) continue;
#pragma unroll
            for (int j = 0; j < KS; ++j)
#pragma unroll
                for (int i = 0; i < NBn; ++i)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) mma_k16(fb[tp][j][i], fa[tp][j][mb], acc[mb][i], T());
        }
#ifndef STEP_EMUL
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
#endif
        __syncthreads();
    };
    if (grp == 1) __syncthreads();                         // anti-phase: group 1 runs one phase behind group 0
    static_for<SPS>([&](auto si) { step(si); });
    if (grp == 0) __syncthreads();

    // ---- epilogue: conv_tap_body's 16-bit one (transposed accumulators: a lane owns ONE pixel and, per register quad, four consecutive
    // channels; one lane swap per dword pair gives every lane 16 contiguous bytes), all NBn blocks of the one channel group
    T* yg = (T*)p.y;
    long long opix[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        int tdl, thl, twl;
        const bool inbox = tile_pix(m0 + mb * 32 + (lane & 31), tdl, thl, twl);
        const int od = d0 + tdl, oh = h0 + thl, ow = w0 + twl;
        opix[mb] = (inbox && od < p.D && oh < p.H && ow < p.W) ? (((long long)n * p.D + od) * p.H + oh) * p.W + ow : -1;
    }
    if (p.vec_epi) {
#pragma unroll
        for (int i = 0; i < NBn; ++i) {
            const int cl = i * 32;
            f32x4 sc[4], sh[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                sc[g] = *(const f32x4*)(ldsS + cl + 8 * g + 4 * khalf);
                sh[g] = *(const f32x4*)(ldsS + NBn * 32 + cl + 8 * g + 4 * khalf);
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const bool okp = opix[mb] >= 0;
                const size_t obase = (size_t)(okp ? opix[mb] : 0);
                unsigned d[4][2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[mb][i][4 * g + e] * sc[g][e] + sh[g][e];
                    if (p.relu) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = relu_nan(v[e]);
                    }
                    d[g][0] = (unsigned)elem<T>::bits16(v[0]) | ((unsigned)elem<T>::bits16(v[1]) << 16);
                    d[g][1] = (unsigned)elem<T>::bits16(v[2]) | ((unsigned)elem<T>::bits16(v[3]) << 16);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    lane32_swap(d[2 * h][0], d[2 * h + 1][0]);
                    lane32_swap(d[2 * h][1], d[2 * h + 1][1]);
                    const int co = cl + 16 * h + 8 * khalf;
                    if (okp && co < p.Cout) {
                        const u32x4 o = {d[2 * h][0], d[2 * h][1], d[2 * h + 1][0], d[2 * h + 1][1]};
                        *(u32x4*)(yg + obase * p.y_cstride + p.y_coff + co) = o;
                    }
                }
            }
        }
        return;
    }
    // channel counts / offsets off the 16-byte grid: element stores (same ownership)
#pragma unroll
    for (int i = 0; i < NBn; ++i) {
        const int cl = i * 32;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cl + cd_row(r, lane);
                if (opix[mb] >= 0 && co < p.Cout) {
                    const size_t o = (size_t)opix[mb];
                    float v = acc[mb][i][r] * ldsS[co] + ldsS[NBn * 32 + co];
                    if (p.relu) v = relu_nan(v);
                    yg[o * p.y_cstride + p.y_coff + co] = elem<T>::from_f32(v);
                }
            }
        }
    }
}

// LDS of conv_tap_body<T, 0, NB, 3, 3, 3, 2, 2, 8, 1, true> (general boxes, two-phase, no fused input): halo | two groups x two half-step
// buffers | scale table (checked against the body's own sum by its static_assert on EXTB)
__host__ __device__ constexpr int conv_tap_group_lds_bytes(int nb) { return conv_gen_npix(8, nb) * 80 + 2 * 2 * 2 * (nb * 2 * 1024) + 2 * nb * 32 * 2 * 4; }
__host__ __device__ constexpr int narrow_arena_bytes(int nb) {
    int a = conv_tap_group_lds_bytes(nb);
    if (NARROW_LDS_BYTES > a) a = NARROW_LDS_BYTES;
    return a;
}

// a narrow member's workgroup: NBn = its channel blocks (whatever the wide partner's NB), KS from its Cin
template <typename T>
__device__ __forceinline__ void conv_tap_narrow_dispatch(const ConvParams& p, unsigned char* arena) {
    const int key = p.nblk32 * 2 + (p.Cin <= 16 ? 0 : 1);   // (uniform: scalar branches)
    if (key == 2) conv_tap_narrow_body<T, 1, 1>(p, arena);
    else if (key == 3) conv_tap_narrow_body<T, 1, 2>(p, arena);
    else if (key == 4) conv_tap_narrow_body<T, 2, 1>(p, arena);
    else if (key == 5) conv_tap_narrow_body<T, 2, 2>(p, arena);
    else if (key == 6) conv_tap_narrow_body<T, 3, 1>(p, arena);
    else if (key == 7) conv_tap_narrow_body<T, 3, 2>(p, arena);
}

// conv_tap_group_kernel / conv_tap_group_pw_kernel with the narrow form for the members marked p.narrow: same grid layout (every member its
// contiguous blockIdx.x range, longest first, XCD-aware order inside the range), ONE LDS arena for whichever body a workgroup runs.
template <typename T, int NB>
__global__ __launch_bounds__(512, 2)
void conv_tap_group_kernel_narrow(ConvGroupParams g) {
    constexpr int ARENA = narrow_arena_bytes(NB);
    __shared__ __attribute__((aligned(16))) unsigned char arena[ARENA];
    const int k = (g.n > 1 && blockIdx.x >= (unsigned)g.p[1].gbase) ? 1 : 0;
    if (g.p[k].narrow) conv_tap_narrow_dispatch<T>(g.p[k], arena);
    else conv_tap_body<T, 0, NB, 3, 3, 3, 2, 2, 8, 1, true, false, false, false, ARENA>(g.p[k], arena);
}

template <typename T, int NB>
__global__ __launch_bounds__(512, 2)
void conv_tap_group_pw_kernel_narrow(ConvGroupParams g) {
    constexpr int ARENA = narrow_arena_bytes(NB);
    static_assert(ARENA >= conv_pw_lds_bytes<T, 1, 4>(), "the pointwise body's buffers fit the arena");
    __shared__ __attribute__((aligned(16))) unsigned char arena[ARENA];
    if (blockIdx.x >= (unsigned)g.pw.gbase) {
        if (threadIdx.x < 256) conv_pw_body<T, 1, 4, true>(g.pw, arena);
        return;
    }
    const int k = (g.n > 1 && blockIdx.x >= (unsigned)g.p[1].gbase) ? 1 : 0;
    if (g.p[k].narrow) conv_tap_narrow_dispatch<T>(g.p[k], arena);
    else conv_tap_body<T, 0, NB, 3, 3, 3, 2, 2, 8, 1, true, false, false, false, ARENA>(g.p[k], arena);
}

template <typename T>
int conv_tap_group_narrow_launch_impl(int NB, const ConvGroupParams& g, dim3 grid, step_stream_t stream) {
    if (g.pw.gcount > 0) {
        switch (NB) {
            case 1: STEP_LAUNCH((conv_tap_group_pw_kernel_narrow<T, 1>), grid, dim3(512), stream, g); break;
            case 2: STEP_LAUNCH((conv_tap_group_pw_kernel_narrow<T, 2>), grid, dim3(512), stream, g); break;
            default: STEP_LAUNCH((conv_tap_group_pw_kernel_narrow<T, 3>), grid, dim3(512), stream, g); break;
        }
        return STEP_LAUNCH_CHECK();
    }
    switch (NB) {
        case 1: STEP_LAUNCH((conv_tap_group_kernel_narrow<T, 1>), grid, dim3(512), stream, g); break;
        case 2: STEP_LAUNCH((conv_tap_group_kernel_narrow<T, 2>), grid, dim3(512), stream, g); break;
        default: STEP_LAUNCH((conv_tap_group_kernel_narrow<T, 3>), grid, dim3(512), stream, g); break;
    }
    return STEP_LAUNCH_CHECK();
}

}  // namespace step
