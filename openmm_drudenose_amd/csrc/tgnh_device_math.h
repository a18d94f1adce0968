// tgnh_device_math.h -- what every kernel of csrc/ may use: precision traits, reciprocal / root / absolute value per precision,
// the fixed-point force as a floating-point number, the 64-lane sum.  Included by .hip files only.
#ifndef TGNH_DEVICE_MATH_H_
#define TGNH_DEVICE_MATH_H_
#include "tgnh_internal.h"

namespace tgnh {

template <int PREC> struct Prec;
template <> struct Prec<TGNH_PREC_SINGLE> { typedef float real; typedef float mixed; typedef float4 real4; typedef float4 mixed4; };
template <> struct Prec<TGNH_PREC_MIXED>  { typedef float real; typedef double mixed; typedef float4 real4; typedef double4 mixed4; };
template <> struct Prec<TGNH_PREC_DOUBLE> { typedef double real; typedef double mixed; typedef double4 real4; typedef double4 mixed4; };

__device__ __forceinline__ float4 mk4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
__device__ __forceinline__ double4 mk4(double x, double y, double z, double w) { return make_double4(x, y, z, w); }
__device__ __forceinline__ float rcp_(float x) { return 1.0f / x; }
// fp64 reciprocal of a normal, non-zero number (masses and their sums): hardware seed + two Newton steps, 5
// instructions and <= 1-2 ulp, where the IEEE division is 11 (it also scales denormals and fixes up specials).
__device__ __forceinline__ double rcp_(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ float sqrt_(float x) { return sqrtf(x); }
__device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
__device__ __forceinline__ float abs_(float x) { return fabsf(x); }
__device__ __forceinline__ double abs_(double x) { return fabs(x); }

// Sum over the 64 lanes of a wavefront, the same value (and the same bits) in every lane.  Data-parallel-primitive moves
// inside the vector ALU -- quads, then rows of 16 (row_shr 4, 8), then row broadcasts; the total lands in lane 63 and is read
// back as a scalar -- instead of six __shfl_xor butterflies: a shuffle is two ds_bpermute_b32 through the LDS crossbar per
// double, ~100 cycles of latency per step, and these sums (the kinetic-energy bins at the end of a pass, the rows collected by
// work-group 0) sit on the path every work-group of a launch waits for.  The order of the additions is fixed.
#ifndef TGNH_WAVE_SUM_DPP
#define TGNH_WAVE_SUM_DPP 1
#endif
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(const double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);   // lanes without a source: +0.0
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
#if TGNH_WAVE_SUM_DPP
    v = dpp_add<0xb1, 0xf>(v);       // quad_perm:[1,0,3,2]
    v = dpp_add<0x4e, 0xf>(v);       // quad_perm:[2,3,0,1]: every lane of a quad holds the quad's sum
    v = dpp_add<0x114, 0xf>(v);      // row_shr:4
    v = dpp_add<0x118, 0xf>(v);      // row_shr:8: lane 15 of every row holds the row's sum
    v = dpp_add<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3: lane 63 holds the total
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
#else
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
#endif
}

// (mixed)force: the fixed-point force as a floating-point number, rounded once.  For doubles hi 2^32 + lo in one fma --
// both parts are exact, so this is the correctly rounded conversion (the bits of the cast) in 3 instructions instead of 4.
__device__ __forceinline__ double force_as(const long long f, double) {
    return fma((double)(int)(f >> 32), 4294967296.0, (double)(unsigned)f);
}
__device__ __forceinline__ float force_as(const long long f, float) { return (float)f; }

}  // namespace tgnh
#endif
