// tgnh_virtual_sites.hip -- the kernels behind tgnh_compute_virtual_sites / tgnh_distribute_virtual_site_forces: the library's own
// virtual-site stage for a host that has no OpenMM behind it (the glue keeps calling OpenMM's computeVirtualSites, Cu :377); the
// harness' site_kernel (tgnh_harness.hip) stays beside it.  The four kinds are OpenMM's; with x1, x2, x3 the parents' positions
// (posq, + posq_correction in mixed precision) and r1k = xk - x1:
//   two-particle average      w1 x1 + w2 x2
//   three-particle average    (w1 x1 + w2 x2) + w3 x3
//   out of plane              ((x1 + w12 r12) + w13 r13) + wc (r12 x r13)
//   local coordinates         o + px X + py Y + pz Z;  o = sum wo x, a = sum wx x, b = sum wy x, c = a x b, X = a / |a|, Z = c / |c|, Y = Z x X
// Everything in fp64 in every precision, every operation rounded on its own (no fused multiply-add, in the order written: a test
// restates the averages in numpy and asks for the same bits).
//
// PLACEMENT: one lane per site, rows sorted by site slot; x, y, z of the site's slot are written -- mixed precision: the fp32 value
// and the residual into posq_correction; single: rounded once -- by stores of those three components alone: the slot is not read.
// DISTRIBUTION: tgnh_receiver_device.h's form, one lane per RECEIVING slot, but one lane per row of the inverse with no grid-stride
// loop (vs_grid).  Per entry of the slot's list the lane reads the site's fixed-point force, f = F / 2^32, and forms this parent's
// share: the transpose of the placement's Jacobian at the current parent positions applied to f.  A parent is never a site (the
// host checked), so no lane reads an entry another lane writes.  A site's frame is computed once per receiving parent: arithmetic,
// not traffic.
//   averages             w_m f
//   out of plane         f2 = w12 f + wc (r13 x f), f3 = w13 f - wc (r12 x f), f1 = f - f2 - f3
//   local coordinates    with u_X = px f + py (f x Z), u_Z = pz f + py (X x f) (the gradients with respect to X and Z),
//                        t_a = (u_X - (u_X . X) X) / |a|, t_c = (u_Z - (u_Z . Z) Z) / |c| (through the two normalisations),
//                        g_a = t_a + b x t_c, g_b = t_c x a (through the cross product):  f_m = wo_m f + wx_m g_a + wy_m g_b
// A degenerate frame (a parallel to b) divides by zero and stores what comes out.  No LDS, no atomic, no inline assembly.
#include "tgnh_virtual_sites.h"
#include "tgnh_receiver_device.h"      // Fixed3, add_to_planes; Vec3 and a parent's position as include/drude_tgnh.h defines it (slot_position)

namespace tgnh {

#pragma clang fp contract(off)

__device__ __forceinline__ double vs_param(const SiteTable& t, const int k, const int row) { return t.params[(size_t)k * t.n + row]; }
__device__ __forceinline__ Vec3 vs_param3(const SiteTable& t, const int k, const int row) { return {vs_param(t, k, row), vs_param(t, k + 1, row), vs_param(t, k + 2, row)}; }
__device__ __forceinline__ Vec3 vs_weighted(const Vec3 w, const Vec3 x1, const Vec3 x2, const Vec3 x3) { return (w.x * x1 + w.y * x2) + w.z * x3; }

// the frame of a local-coordinates site: what placement and distribution both need
struct VsFrame { Vec3 a, b, X, Y, Z; double inv_a, inv_c; };
__device__ __forceinline__ VsFrame vs_frame(const Vec3 wx, const Vec3 wy, const Vec3 x1, const Vec3 x2, const Vec3 x3) {
    VsFrame fr;
    fr.a = vs_weighted(wx, x1, x2, x3);
    fr.b = vs_weighted(wy, x1, x2, x3);
    const Vec3 c = cross(fr.a, fr.b);
    fr.inv_a = 1.0 / sqrt(dot(fr.a, fr.a));
    fr.inv_c = 1.0 / sqrt(dot(c, c));
    fr.X = fr.inv_a * fr.a;
    fr.Z = fr.inv_c * c;
    fr.Y = cross(fr.Z, fr.X);
    return fr;
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void place_sites_kernel(const SitePlaceArgs a) {
    typedef typename Prec<PREC>::real real;
    typedef typename Prec<PREC>::real4 real4;
    const int row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= a.t.n) return;
    const int4 at = a.t.atoms[row];
    const int kind = a.t.kind[row];
    const Vec3 x1 = slot_position<PREC>(a.posq, a.posq_corr, at.y), x2 = slot_position<PREC>(a.posq, a.posq_corr, at.z);
    // the third parent and the first three planes are read whatever the kind, so that no load waits for the branch on the kind word (a
    // two-particle site: p3 = -1 reads p2 again, and the third plane holds the host's zero; neither is used)
    const Vec3 x3 = slot_position<PREC>(a.posq, a.posq_corr, at.w >= 0 ? at.w : at.z);
    const Vec3 w = vs_param3(a.t, 0, row);
    Vec3 s;
    if (kind == VS_TWO_AVERAGE) {
        s = w.x * x1 + w.y * x2;
    } else {
        if (kind == VS_THREE_AVERAGE) {
            s = vs_weighted(w, x1, x2, x3);
        } else if (kind == VS_OUT_OF_PLANE) {
            const Vec3 r12 = x2 - x1, r13 = x3 - x1;
            s = ((x1 + w.x * r12) + w.y * r13) + w.z * cross(r12, r13);
        } else {
            const VsFrame fr = vs_frame(vs_param3(a.t, 3, row), vs_param3(a.t, 6, row), x1, x2, x3);
            const Vec3 p = vs_param3(a.t, 9, row);
            s = ((vs_weighted(w, x1, x2, x3) + p.x * fr.X) + p.y * fr.Y) + p.z * fr.Z;
        }
    }
    // x, y, z alone are stored (12 or 24 of the slot's 16 or 32 bytes): the slot's w is not read, and stays
    real* o = reinterpret_cast<real*>(static_cast<real4*>(a.posq) + at.x);
    const real hx = (real)s.x, hy = (real)s.y, hz = (real)s.z;
    o[0] = hx; o[1] = hy; o[2] = hz;
    if (PREC == TGNH_PREC_MIXED) {
        float* c = reinterpret_cast<float*>(static_cast<float4*>(a.posq_corr) + at.x);
        c[0] = (float)(s.x - (double)hx); c[1] = (float)(s.y - (double)hy); c[2] = (float)(s.z - (double)hz);
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void spread_site_forces_kernel(const SiteSpreadArgs a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= a.recv.n) return;
    const int slot = a.recv.slot[r];
    const int e1 = a.recv.start[r + 1];
    Fixed3 sum = {0, 0, 0};                                      // (written out: `Fixed3 sum;` schedules the kernel's instructions in another order)
    for (int e = a.recv.start[r]; e < e1; e++) {
        const int row = a.recv.term[e], role = a.recv.role[e];
        const int4 at = a.t.atoms[row];
        const int kind = a.t.kind[row];
        const Vec3 f = {(double)a.force[at.x] * (1.0 / 4294967296.0), (double)a.force[(size_t)a.padded + at.x] * (1.0 / 4294967296.0),
                        (double)a.force[2 * (size_t)a.padded + at.x] * (1.0 / 4294967296.0)};
        Vec3 share;
        if (kind == VS_TWO_AVERAGE || kind == VS_THREE_AVERAGE) {
            share = vs_param(a.t, role, row) * f;
        } else {
            const Vec3 x1 = slot_position<PREC>(a.posq, a.posq_corr, at.y), x2 = slot_position<PREC>(a.posq, a.posq_corr, at.z),
                       x3 = slot_position<PREC>(a.posq, a.posq_corr, at.w);
            if (kind == VS_OUT_OF_PLANE) {
                const Vec3 w = vs_param3(a.t, 0, row), r12 = x2 - x1, r13 = x3 - x1;
                const Vec3 f2 = w.x * f + w.z * cross(r13, f), f3 = w.y * f - w.z * cross(r12, f);
                share = role == 1 ? f2 : (role == 2 ? f3 : (f - f2) - f3);
            } else {
                const VsFrame fr = vs_frame(vs_param3(a.t, 3, row), vs_param3(a.t, 6, row), x1, x2, x3);
                const Vec3 p = vs_param3(a.t, 9, row);
                const Vec3 uX = p.x * f + p.y * cross(f, fr.Z), uZ = p.z * f + p.y * cross(fr.X, f);
                const Vec3 ta = fr.inv_a * (uX - dot(uX, fr.X) * fr.X), tc = fr.inv_c * (uZ - dot(uZ, fr.Z) * fr.Z);
                const Vec3 ga = ta + cross(fr.b, tc), gb = cross(tc, fr.a);
                share = (vs_param(a.t, role, row) * f + vs_param(a.t, 3 + role, row) * ga) + vs_param(a.t, 6 + role, row) * gb;
            }
        }
        sum.add(share);
    }
    add_to_planes(a.force, a.padded, slot, sum);
}

static bool vs_table_ok(const SiteTable& t) { return t.n >= 1 && t.atoms && t.kind && t.params; }

hipError_t launch_place_sites(int precision, const SitePlaceArgs& a, hipStream_t s) {
    if (!vs_table_ok(a.t) || !a.posq || (precision == TGNH_PREC_MIXED && !a.posq_corr)) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(place_sites_kernel, precision, dim3(vs_grid(a.t.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_spread_site_forces(int precision, const SiteSpreadArgs& a, hipStream_t s) {
    if (!vs_table_ok(a.t) || !receivers_ok(a.recv) || !a.posq || !a.force || a.padded < 1 ||
        (precision == TGNH_PREC_MIXED && !a.posq_corr))
        return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(spread_site_forces_kernel, precision, dim3(vs_grid(a.recv.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace tgnh
