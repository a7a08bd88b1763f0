// step_amd/csrc/pool_vec.h -- 16-byte channel vectors and their element-wise max in the storage type (the pool kernels of pool.hip).
#pragma once
#include "common.h"

namespace step {

template <typename T, int V> struct Vec16;
template <> struct Vec16<float, 4> {
    typedef f32x4 raw;
    __device__ static __forceinline__ void unpack(const raw& r, float (&f)[4]) { for (int i = 0; i < 4; ++i) f[i] = r[i]; }
    __device__ static __forceinline__ raw pack(const float (&f)[4]) { raw r = {f[0], f[1], f[2], f[3]}; return r; }
};
template <typename T> struct Vec16h {
    typedef u16x8 raw;
    __device__ static __forceinline__ void unpack(const raw& r, float (&f)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { T e; e.v = r[i]; f[i] = elem<T>::to_f32(e); }
    }
    __device__ static __forceinline__ raw pack(const float (&f)[8]) {
        raw r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = elem<T>::from_f32(f[i]).v;
        return r;
    }
};
template <> struct Vec16<bf16_t, 8> : Vec16h<bf16_t> {};
template <> struct Vec16<f16_t, 8> : Vec16h<f16_t> {};


// element-wise max of two 16-byte channel vectors in the storage type (the max of two representable
// values is representable: no rounding anywhere in a max pool).  enc / dec map a vector to and from the
// form the max is taken in.  The max PROPAGATES a NaN of either sign (the non-finite contract of common.h),
// by the same rule in all three storage types and in the host interpreter.  (Forward pools only: the
// backward kernels walk their windows with `val > max`, which skips a NaN, and share nothing with this.)
template <typename T> struct VecMax;
template <> struct VecMax<float> {
    __device__ static __forceinline__ f32x4 enc(const f32x4& a) { return a; }
    __device__ static __forceinline__ f32x4 dec(const f32x4& a) { return a; }
    __device__ static __forceinline__ f32x4 lowest() { const float m = -__builtin_inff(); f32x4 r = {m, m, m, m}; return r; }
    __device__ static __forceinline__ f32x4 max(const f32x4& a, const f32x4& b) {          // v_maximum3_f32
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = max_nan(a[i], b[i]);
        return r;
    }
};
#ifndef STEP_EMUL
template <> struct VecMax<f16_t> {
    __device__ static __forceinline__ u16x8 enc(const u16x8& a) { return a; }
    __device__ static __forceinline__ u16x8 dec(const u16x8& a) { return a; }
    __device__ static __forceinline__ u16x8 lowest() { u16x8 r; for (int i = 0; i < 8; ++i) r[i] = 0xfc00; return r; }   // -inf
    __device__ static __forceinline__ u16x8 max(const u16x8& a, const u16x8& b) {          // v_pk_maximum3_f16 (v_pk_max_f16 drops a NaN)
        return __builtin_bit_cast(u16x8, __builtin_elementwise_maximum(__builtin_bit_cast(f16x8_hw, a), __builtin_bit_cast(f16x8_hw, b)));
    }
};
template <> struct VecMax<bf16_t> {
    // gfx950 has no packed bf16 max, and widening to fp32 costs ~9 VALU ops per pair (measured: the pool was
    // VALU-bound), so planes are re-keyed once when they enter LDS, every max is one v_pk_max_i16 per pair, and
    // the same map -- an involution -- brings the result back before the store.  The key of a pattern x, as a
    // two's-complement integer:  x for x >= +0,  0x7f80 - x (mod 2^16) for the negative ones: -0 -> -128, larger
    // magnitudes below it, -inf -> -32768 (no key is lower), and the negative NaNs 0xff81 .. 0xffff -> 0x7fff ..
    // 0x7f81, ABOVE +inf where the positive NaNs are: a NaN of either sign wins every max and comes back as a NaN.
    // Per pair of elements: m = x >> 15 (arithmetic), key = (x ^ m) + (m & 0x7f81) -- v_pk_ashrrev_i16, v_and_b32 and
    // ONE 32-bit v_xad_u32, because the sum never carries out of a 16-bit half (~x <= 0x7fff for a negative x).
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    __device__ static __forceinline__ u16x8 enc(const u16x8& a) {
        const u32x4 x = __builtin_bit_cast(u32x4, a);
        const u32x4 m = __builtin_bit_cast(u32x4, __builtin_bit_cast(s16x8, a) >> 15);
        return __builtin_bit_cast(u16x8, (x ^ m) + (m & 0x7f817f81u));
    }
    __device__ static __forceinline__ u16x8 dec(const u16x8& k) { return enc(k); }
    __device__ static __forceinline__ u16x8 lowest() { u16x8 r; for (int i = 0; i < 8; ++i) r[i] = 0x8000; return r; }   // the key of -inf: no key is lower
    __device__ static __forceinline__ u16x8 max(const u16x8& a, const u16x8& b) {
        return __builtin_bit_cast(u16x8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b)));
    }
};
#else
template <typename T> struct VecMax {
    __device__ static inline u16x8 enc(const u16x8& a) { return a; }
    __device__ static inline u16x8 dec(const u16x8& a) { return a; }
    __device__ static inline u16x8 lowest() {                                  // -inf in the storage type
        float f[8];
        for (int i = 0; i < 8; ++i) f[i] = -__builtin_inff();
        return Vec16<T, 8>::pack(f);
    }
    __device__ static inline u16x8 max(const u16x8& a, const u16x8& b) {
        float fa[8], fb[8];
        Vec16<T, 8>::unpack(a, fa); Vec16<T, 8>::unpack(b, fb);
        for (int i = 0; i < 8; ++i) fa[i] = max_nan(fa[i], fb[i]);
        return Vec16<T, 8>::pack(fa);
    }
};
#endif

}  // namespace step
