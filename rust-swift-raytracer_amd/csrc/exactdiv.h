// exactdiv.h -- correctly rounded f32 division and reciprocal for gfx950
// without HIP's general divide expansion (v_div_scale x2, v_rcp, 5 fma,
// v_div_fmas, v_div_fixup per quotient).
//
// The reference divides with plain Rust f32 `/` (IEEE, correctly rounded):
// NVec3::new's three divisions by the length (maths.rs:111-118), the normal's
// `/ radius` (common.rs:95) and the camera's `/ (W-1)`, `/ (H-1)`
// (common.rs:335-336).  A quotient a/b computed here is the same bits:
//
//   y  = RN(1/b)            v_rcp_f32 (<= 1 ulp) + one Newton step with fma
//   q  = RN(a*y)            within 1 ulp of a/b
//   r  = RN(q*b - a)        exact (fma; the remainder is representable)
//   q' = RN(q - r*y)        Markstein's theorem: q' == RN(a/b)
//
// Markstein (IBM J. R&D 34(1), 1990; Muller et al., Handbook of
// Floating-Point Arithmetic, 2nd ed., Thm 4.10): if y is 1/b correctly
// rounded and q is within one ulp of a/b, the corrected quotient is a/b
// correctly rounded, provided no step under- or overflows.  The guards below
// keep every operand in that range (denominator in [2^-40, 2^40], numerator
// 0 or of magnitude in [2^-60, 2^60]: then |q| >= 2^-100 and the remainder's
// quantum is >= 2^-149) and callers fall back to the HIP divide otherwise.
// The one step rcp -> RN(1/b) is not covered by the theorem for every
// hardware rcp result, so it is checked exhaustively on the device for every
// b in the guarded range (tools/exactdiv_check.hip, tests/test_gpu_exactdiv.py).
//
// Signed zeros: with r = q*b - a and q' = q - r*y (rather than r = a - q*b,
// q' = q + r*y) a zero numerator keeps its sign for b > 0, as IEEE division
// does; b > 0 is part of the denominator guard.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtamd {

// b in [2^-40, 2^40] (so also b > 0, finite, not NaN): one unsigned compare.
__device__ __forceinline__ bool xdiv_den_ok(float b) {
    return (__float_as_uint(b) - 0x2B800000u) <= (0x53800000u - 0x2B800000u);
}

// a == 0 or |a| in [2^-60, 2^60) for three numerators (frexp exponent of 0 is 0;
// of inf/NaN it is 0 as well, which the magnitude test rejects: a sum, not a
// max, because fmaxf drops NaN operands).
__device__ __forceinline__ bool xdiv_num3_ok(float a, float b, float c) {
    const int e = min(min(__builtin_amdgcn_frexp_expf(a), __builtin_amdgcn_frexp_expf(b)),
                      __builtin_amdgcn_frexp_expf(c));
    const float m = (fabsf(a) + fabsf(b)) + fabsf(c);
    return (e >= -59) & (m < 0x1p60f);
}

// The same guard for numerators bounded by the denominator (|a| <= b (1 +
// 2^-22), as the components of a vector are by its computed length): with b
// <= 2^40 the upper bound holds by itself, so only the exponents are checked
// (0 and inf/NaN have frexp exponent 0; inf/NaN components make the length
// fail xdiv_den_ok).
__device__ __forceinline__ bool xdiv_num3_small_ok(float a, float b, float c) {
    const int e = min(min(__builtin_amdgcn_frexp_expf(a), __builtin_amdgcn_frexp_expf(b)),
                      __builtin_amdgcn_frexp_expf(c));
    return e >= -59;
}

// RN(1/b) for b in the guarded range (exhaustively checked, see above).
__device__ __forceinline__ float xdiv_rcp(float b) {
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, y0, 1.0f);
    return __builtin_fmaf(e, y0, y0);
}

// RN(a/b) given y = RN(1/b), b > 0, within the guards.
__device__ __forceinline__ float xdiv(float a, float b, float y) {
    const float q = a * y;
    const float r = __builtin_fmaf(q, b, -a);
    return __builtin_fmaf(-r, y, q);
}

// RN(sqrt(a)) -- the bits of IEEE sqrtf (maths.rs:107 `f32::sqrt`,
// common.rs:84) without the general expansion's denormal scaling and class
// fix-up.  gfx950's v_sqrt_f32 is within one ulp of the exact root for every
// positive normal input (tools/sqrt_probe.hip), so the correctly rounded root
// is s, s - ulp or s + ulp; the two residuals a - s'*s (one fma each, exact
// enough for a >= 2^-96) pick it, as in the general sequence.  Inputs below
// 2^-96 (and zero, negatives, NaN) take HIP's sqrtf.  Checked on the device
// against sqrtf for all 2^32 inputs (tools/exactdiv_check.hip).
//
// Fallbacks, here and in xdivide3 / xunit3: the fast sequence runs in every
// active lane without a branch (its value in a lane outside the guards is
// never used), and one wave-wide test of the guard (a ballot, so a scalar
// compare and one branch, no exec-mask save and restore) reaches the block
// that computes HIP's result and selects it per lane.  Ordinary scenes never
// enter that block; a wave that does pays for both sequences.
// (the hint stands at the `if` itself: inside a helper it is lowered before
// inlining, where it feeds a return and is lost, and the fallback block then
// stays in the middle of the fast path, which jumps over it)
#define XDIV_ANY_LANE(c) __builtin_expect(__builtin_amdgcn_ballot_w64(c) != 0ull, 0)

// The unguarded sequence: RN(sqrt(a)) for a >= 2^-96.
__device__ __forceinline__ float xsqrt_fast(float a) {
    const float s = __builtin_amdgcn_sqrtf(a);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u);
    const float sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, a);
    const float rp = __builtin_fmaf(-sp, s, a);
    float r = rm <= 0.0f ? sm : s;
    r = rp > 0.0f ? sp : r;
    return r;
}

// kWaveGuard = false, here and below, is the per-lane form: the fallback in a
// divergent region of its own (an exec-mask save and restore around it at
// every site).  The triangle-mesh kernels keep it: they are at their register
// limit, and holding the fast results across the wave-wide test cost two of
// them scratch.
template <bool kWaveGuard = true>
__device__ __forceinline__ float xsqrt(float a) {
    float r = xsqrt_fast(a);
    const bool slow = !(a >= 0x1p-96f);
    if (kWaveGuard) {
        if (XDIV_ANY_LANE(slow)) {
            // (an empty statement the compiler may not move or run ahead of the
            // branch: without it the backend's if-conversion of wave-uniform
            // branches computes sqrtf's expansion, 15 VALU, in every lane of every
            // call and selects with s_cselect / v_cndmask instead of branching)
            float t = a;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(t));
#endif
            r = slow ? __builtin_sqrtf(t) : r;
        }
    } else {
        if (__builtin_expect(slow, 0)) r = __builtin_sqrtf(a);
    }
    return r;
}

// (x, y, z) / b, the bits of three `/`: one shared reciprocal and three
// corrected quotients inside the guards, HIP's divide otherwise.
template <bool kWaveGuard = true>
__device__ __forceinline__ void xdivide3(float &x, float &y, float &z, float b) {
    const bool ok = xdiv_den_ok(b) & xdiv_num3_ok(x, y, z);  // (bitwise: no branch)
    if (!kWaveGuard) {
        if (__builtin_expect(ok, 1)) {
            const float r = xdiv_rcp(b);
            x = xdiv(x, b, r);
            y = xdiv(y, b, r);
            z = xdiv(z, b, r);
        } else {
            x = x / b;
            y = y / b;
            z = z / b;
        }
        return;
    }
    const float r = xdiv_rcp(b);
    float qx = xdiv(x, b, r), qy = xdiv(y, b, r), qz = xdiv(z, b, r);
    if (XDIV_ANY_LANE(!ok)) {
        const float sx = x / b, sy = y / b, sz = z / b;
        qx = ok ? qx : sx;
        qy = ok ? qy : sy;
        qz = ok ? qz : sz;
    }
    x = qx;
    y = qy;
    z = qz;
}

// NVec3::new (maths.rs:111-118): (x, y, z) / sqrt((x*x + y*y) + z*z).  The
// components are bounded by the length, so the cheaper numerator guard does.
//
// One guard for the root and the quotients.  The length is the unguarded
// root; when it fails xdiv_den_ok (outside [2^-40, 2^40], or NaN) or a
// component fails its guard, the fallback block takes the length from sqrtf
// and divides with `/`, so nothing of the fast sequence is used.  When the
// fast root len passes, len >= 2^-40, and v_sqrt_f32 being within one ulp and
// the residual step moving it by at most one more puts the exact root above
// 2^-40 (1 - 2^-22), so the sum is >= 2^-81 > 2^-96, where xsqrt_fast is the
// exact root: xsqrt's own guard could not have fired.  That covers normal
// inputs; that no zero, denormal, negative or NaN sum yields a fast root
// inside [2^-40, 2^40] is checked with every other input: for all 2^32 sums
// `den_ok(fast) ? fast : sqrtf` has the bits of sqrtf (tools/exactdiv_check.hip).
template <bool kWaveGuard = true>
__device__ __forceinline__ void xunit3(float &x, float &y, float &z) {
#pragma clang fp contract(off)
    const float n = (x * x + y * y) + z * z;
    if (!kWaveGuard) {  // (the root with its own guard, then the quotients')
        const float len = xsqrt<false>(n);
        if (__builtin_expect(xdiv_den_ok(len) & xdiv_num3_small_ok(x, y, z), 1)) {
            const float r = xdiv_rcp(len);
            x = xdiv(x, len, r);
            y = xdiv(y, len, r);
            z = xdiv(z, len, r);
        } else {
            x = x / len;
            y = y / len;
            z = z / len;
        }
        return;
    }
    const float len = xsqrt_fast(n);
    const bool ok = xdiv_den_ok(len) & xdiv_num3_small_ok(x, y, z);
    const float r = xdiv_rcp(len);
    float qx = xdiv(x, len, r), qy = xdiv(y, len, r), qz = xdiv(z, len, r);
    if (XDIV_ANY_LANE(!ok)) {
        const float slen = __builtin_sqrtf(n);
        const float sx = x / slen, sy = y / slen, sz = z / slen;
        qx = ok ? qx : sx;
        qy = ok ? qy : sy;
        qz = ok ? qz : sz;
    }
    x = qx;
    y = qy;
    z = qz;
}

}  // namespace rtamd
