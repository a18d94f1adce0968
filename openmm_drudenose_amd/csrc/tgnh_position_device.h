// tgnh_position_device.h -- a slot's position as include/drude_tgnh.h defines it, in fp64, and the three-vector the units that work
// on such positions share (tgnh_virtual_sites.hip, tgnh_drude_force.hip): written once.  Every operation is rounded on its own, in the
// order written (the including unit says `#pragma clang fp contract(off)`; tests restate some of these in numpy and ask for the same
// bits).  Included by .hip files only, by none of the step kernels' units.
#ifndef TGNH_POSITION_DEVICE_H_
#define TGNH_POSITION_DEVICE_H_
#include "tgnh_device_math.h"

namespace tgnh {

#pragma clang fp contract(off)

struct Vec3 { double x, y, z; };
__device__ __forceinline__ Vec3 operator+(const Vec3 a, const Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Vec3 operator-(const Vec3 a, const Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 operator*(const double s, const Vec3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(const Vec3 a, const Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ Vec3 cross(const Vec3 a, const Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// posq, + posq_correction in mixed precision
template <int PREC>
__device__ __forceinline__ Vec3 slot_position(const void* posq, const void* corr, const int i) {
    const typename Prec<PREC>::real4 p = static_cast<const typename Prec<PREC>::real4*>(posq)[i];
    Vec3 x = {(double)p.x, (double)p.y, (double)p.z};
    if (PREC == TGNH_PREC_MIXED) {
        const float4 c = static_cast<const float4*>(corr)[i];
        x.x = x.x + (double)c.x; x.y = x.y + (double)c.y; x.z = x.z + (double)c.z;
    }
    return x;
}

// cell_coord's two lines: the fractional coordinate in [0, 1) (the reciprocal sums of tgnh_ewald.hip and tgnh_pme.hip)
__device__ __forceinline__ double frac_coord(const double x, const double L) {
    double s = x / L;
    s = s - floor(s);
    return s;
}

}  // namespace tgnh
#endif
