// ctc_xf.hpp -- what the CTC units (ctc.hip, ctc_beam.hip, ctc_align.hip) and the transducer unit (rnnt.hip) share: the extended-range "xf" arithmetic (an f32 mantissa in [0.5, 1)
// with its own int32 exponent; ctc.hip's header says why), the LDS-only barrier and the LDS ceiling of one workgroup.
#pragma once
#include "nntk_common.hpp"

#define CTC_EZERO (-(1 << 28))
#define CTC_THREADS 256
#define CTC_LDS_LIMIT (160 * 1024)

struct xf { float m; int e; };

__device__ __forceinline__ xf xf_zero() { xf r; r.m = 0.0f; r.e = CTC_EZERO; return r; }
__device__ __forceinline__ xf xf_one() { xf r; r.m = 0.5f; r.e = 1; return r; }
__device__ __forceinline__ xf xf_norm(float m, int e) {
    xf r;
    r.m = __builtin_amdgcn_frexp_mantf(m);
    r.e = m == 0.0f ? CTC_EZERO : e + __builtin_amdgcn_frexp_expf(m);
    return r;
}
// (a + b) + c in this order, always: the bits of a row never depend on anything but the row
__device__ __forceinline__ xf xf_add3(xf a, xf b, xf c) {
    const int em = max(a.e, max(b.e, c.e));
    const float m = (ldexpf(a.m, a.e - em) + ldexpf(b.m, b.e - em)) + ldexpf(c.m, c.e - em);
    return xf_norm(m, em);
}
__device__ __forceinline__ xf xf_times_prob(xf v, float p) {
    // the probability as mantissa and exponent too: a denormal p keeps its bits
    return xf_norm(v.m * __builtin_amdgcn_frexp_mantf(p), v.e + __builtin_amdgcn_frexp_expf(p));
}
// v times a factor that is itself mantissa and exponent (rnnt.hip: an emission far below what an f32 holds)
__device__ __forceinline__ xf xf_times(xf v, xf p) { return xf_norm(v.m * p.m, v.e + p.e); }
// the value as a plain f32 scaled by 2^-e0 (0 below the f32 range)
__device__ __forceinline__ float xf_to_float(xf v, int e0) { return ldexpf(v.m, max(v.e - e0, -1000)); }
// a > b: exponent first, then mantissa (both normalised, neither negative); zero, with the lowest exponent, is below everything
__device__ __forceinline__ bool xf_greater(xf a, xf b) { return a.e > b.e || (a.e == b.e && a.m > b.m); }
__device__ __forceinline__ float2 xf_pack(xf v) { return make_float2(v.m, __int_as_float(v.e)); }
__device__ __forceinline__ xf xf_unpack(float2 w) { xf r; r.m = w.x; r.e = __float_as_int(w.y); return r; }

// LDS traffic only: global loads and stores issued before the barrier stay in flight across it
#define CTC_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
