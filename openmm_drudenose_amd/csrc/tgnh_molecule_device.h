// tgnh_molecule_device.h -- what the kernels that walk molecules share (tgnh_scale_positions.hip, tgnh_wrap.hip): a slot as it lies in
// memory and its coordinates as include/drude_tgnh.h defines them, the store of a moved slot, the wavefront's LDS image, and the two
// centroid walks -- a span's lane range from its mask of molecule heads, and the sum over a member list with its n <= 64 and n > 64
// orders of additions.  The sum is written here and nowhere else: every caller gets the same bits.  Included by .hip files only.
#ifndef TGNH_MOLECULE_DEVICE_H_
#define TGNH_MOLECULE_DEVICE_H_

#include "tgnh_device_math.h"
#include "tgnh_scale_positions.h"

namespace tgnh {

// every product, quotient and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

static_assert(BLOCK % 64 == 0 && SP_SPAN_SLOTS == 64, "whole wavefronts; a span is a wavefront's");

// a slot as it lies in memory, and its coordinates as the header defines them
template <int PREC> struct Site {
    typename Prec<PREC>::real4 p;
    float4 c;                                // mixed precision only
    double x, y, z;
};

template <int PREC>
__device__ __forceinline__ void site_load(const void* posq, const void* corr, const int i, Site<PREC>& s) {
    s.p = static_cast<const typename Prec<PREC>::real4*>(posq)[i];
    s.x = (double)s.p.x; s.y = (double)s.p.y; s.z = (double)s.p.z;
    if (PREC == TGNH_PREC_MIXED) {
        s.c = static_cast<const float4*>(corr)[i];
        s.x = s.x + (double)s.c.x; s.y = s.y + (double)s.c.y; s.z = s.z + (double)s.c.z;
    }
}

// x' = x + d in the position type; the snapshot first (where one is asked for), from the registers the slot was read into
template <int PREC>
__device__ __forceinline__ void site_store(void* posq, void* corr, void* snap_posq, void* snap_corr, const int i, const Site<PREC>& s,
                                           const double dx, const double dy, const double dz) {
    typedef typename Prec<PREC>::real4 R4;
    typedef typename Prec<PREC>::real R;
    if (snap_posq) {
        static_cast<R4*>(snap_posq)[i] = s.p;
        if (PREC == TGNH_PREC_MIXED) static_cast<float4*>(snap_corr)[i] = s.c;
    }
    const double nx = s.x + dx, ny = s.y + dy, nz = s.z + dz;
    const R hx = (R)nx, hy = (R)ny, hz = (R)nz;
    static_cast<R4*>(posq)[i] = mk4(hx, hy, hz, s.p.w);
    if (PREC == TGNH_PREC_MIXED)
        static_cast<float4*>(corr)[i] = make_float4((float)(nx - (double)hx), (float)(ny - (double)hy), (float)(nz - (double)hz), s.c.w);
}

// what a wavefront has written to its LDS image is read by other lanes of the same wavefront
__device__ __forceinline__ void wave_image_ready() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct SpImage { double v[SP_WAVES][3][64]; };       // 6 KiB a work-group: x, y, z of a wavefront's 64 lanes, each wavefront its own

// a span's walk: this lane's molecule runs from the last head at or below the lane to the next head above it (or the span's end)
__device__ __forceinline__ void span_molecule(const unsigned long long heads, const int lane, const int len, int& m0, int& m1) {
    const unsigned long long below = heads & ((2ull << lane) - 1ull);            // (lane 63: 2 << 63 wraps to 0, the mask to all ones)
    m0 = 63 - __clzll((long long)below);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    m1 = above ? min(lane + __ffsll((long long)above), len) : len;
}

// S of the image's lanes [m0, m1): ascending, left to right from the first member's value
__device__ __forceinline__ void image_sum(const double (&im)[3][64], const int m0, const int m1, double& sx, double& sy, double& sz) {
    sx = im[0][m0]; sy = im[1][m0]; sz = im[2][m0];
    for (int k = m0 + 1; k < m1; k++) { sx = sx + im[0][k]; sy = sy + im[1][k]; sz = sz + im[2][k]; }
}

// S of a member list, by a whole wavefront (all 64 lanes arrive; every lane leaves with the same bits): up to 64 members into the
// LDS image, summed in the order above; beyond, lane l adds members l, l + 64, ... in ascending order and the lanes meet in wave_sum
template <int PREC>
__device__ __forceinline__ void members_sum(const void* posq, const void* corr, const int* members, const int b, const int n, const int lane,
                                            double (&im)[3][64], double& sx, double& sy, double& sz) {
    Site<PREC> s;
    if (n <= 64) {
        s.x = s.y = s.z = 0.0;
        if (lane < n) site_load<PREC>(posq, corr, members[b + lane], s);
        im[0][lane] = s.x; im[1][lane] = s.y; im[2][lane] = s.z;
        wave_image_ready();
        image_sum(im, 0, n, sx, sy, sz);                             // (every lane: the same additions)
    } else {
        double tx = 0.0, ty = 0.0, tz = 0.0;
        for (int k = lane; k < n; k += 64) {
            site_load<PREC>(posq, corr, members[b + k], s);
            tx = tx + s.x; ty = ty + s.y; tz = tz + s.z;
        }
        sx = wave_sum(tx); sy = wave_sum(ty); sz = wave_sum(tz);      // (all 64 lanes are here: n is the wavefront's)
    }
}

}  // namespace tgnh

#endif
