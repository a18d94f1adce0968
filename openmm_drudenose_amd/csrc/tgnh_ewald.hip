// tgnh_ewald.hip -- the kernels behind tgnh_set_nonbonded_ewald: what tgnh_compute_nonbonded_force adds to the direct-space erfc pairs
// (tgnh_nonbonded.hip's pair kernels in their Ewald instantiation) when Ewald summation is on, and tgnh_get_ewald_energy's sum.
// include/drude_tgnh.h writes the terms one operation a line; this file follows it.  Everything in fp64 in every precision, every
// operation rounded on its own (no fused multiply-add); erf, exp and sincospi are the device library's.
//
// THE EXCLUSION CORRECTION.  tgnh_receiver_device.h's form: one lane per receiving slot over the table of charged exception rows
// inverted at set time; no cutoff, no periodic image.  A pair at r2 == 0 (a Drude particle on its parent) gives no force and the
// limit of the energy.
// THE RECIPROCAL PART, three launches:
//   ew_sum_kernel       a lane per reciprocal vector, 64 to a wavefront, NB_WAVES tiles to a work-group; the grid is (tiles of vectors)
//                       x (parts of EW_PART consecutive slots).  A wavefront streams its part's (sx, sy, sz, q) through its own LDS
//                       image, 64 slots at a time, without a work-group barrier; every lane reads the same slot (a broadcast) and adds
//                       q cos, q sin to its C and S in slot order.  One (C, S) goes out per (part, vector).
//   ew_finalise_kernel  a lane per vector (index_grid's grid-stride loop): the parts in order, A and k from the box of the call,
//                       (A C, A S, k) for the force launch; with want_energy a row of A (C C + S S) per work-group (tgnh_rows_device.h)
//   ew_force_kernel     a lane per slot, a loop over all vectors in table order: their coefficients are the same for every lane
//                       (uniform loads); one sincospi per (slot, vector) on the reduced phase; each component is converted once
// The phase factor is sincospi(2 t) of the phase in turns, t = (nx sx + ny sy) + nz sz with s the fractional coordinate in [0, 1):
// its reduction is exact and needs no private memory.  No atomic anywhere; every sum's order depends on n, M and the tables alone.
#include "tgnh_ewald.h"
#include "tgnh_receiver_device.h"
#include "tgnh_rows_device.h"

namespace tgnh {

#pragma clang fp contract(off)

namespace {
constexpr double EW_FIXED = 4294967296.0;

// what a wavefront has written to its LDS image is read by other lanes of the same wavefront (and the other way round)
__device__ __forceinline__ void ew_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct EwImage { double v[NB_WAVES][4][64]; };                 // 8 KiB a work-group; each wavefront its own
}  // namespace

template <int PREC>
__global__ __launch_bounds__(BLOCK) void ew_sum_kernel(const EwaldArgs a) {
    __shared__ EwImage img;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = (int)blockIdx.x * BLOCK + (int)threadIdx.x;             // (a wavefront's 64 lanes: one tile of consecutive vectors)
    if ((int)blockIdx.x * BLOCK + w * 64 >= a.m) return;                  // a spare wavefront leaves; nobody waits for it
    const bool active = m < a.m;
    const int4 kv = a.kvec[active ? m : a.m - 1];
    const double nx = (double)kv.x, ny = (double)kv.y, nz = (double)kv.z;
    const int part = blockIdx.y;
    const int first = part * EW_PART, last = min(first + EW_PART, a.n);
    double C = 0.0, S = 0.0;
    for (int base = first; base < last; base += 64) {
        const int count = min(64, last - base);
        ew_wave_sync();                                          // the image's last readers are done
        if (lane < count) {
            const int j = base + lane;
            const Vec3 x = slot_position<PREC>(a.posq, a.posq_corr, j);
            img.v[w][0][lane] = frac_coord(x.x, a.box[0]);
            img.v[w][1][lane] = frac_coord(x.y, a.box[1]);
            img.v[w][2][lane] = frac_coord(x.z, a.box[2]);
            img.v[w][3][lane] = a.par[3 * (size_t)j];
        }
        ew_wave_sync();
        for (int k = 0; k < count; k++) {
            const double t = (nx * img.v[w][0][k] + ny * img.v[w][1][k]) + nz * img.v[w][2][k];
            const double q = img.v[w][3][k];
            double sn, cs;
            sincospi(2.0 * t, &sn, &cs);
            C = C + q * cs;
            S = S + q * sn;
        }
    }
    if (active) a.part_rows[(size_t)part * a.m + m] = make_double2(C, S);
}

template <bool ENERGY>
__device__ __forceinline__ void finalise_body(const EwaldArgs& a, double& e) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.m; it += (long long)gridDim.x * BLOCK) {
        const int m = (int)it;
        double C = 0.0, S = 0.0;
        for (int p = 0; p < a.parts; p++) {
            const double2 r = a.part_rows[(size_t)p * a.m + m];
            C = C + r.x;
            S = S + r.y;
        }
        const int4 kv = a.kvec[m];
        const double kx = ((2.0 * EW_PI) * (double)kv.x) / a.box[0];
        const double ky = ((2.0 * EW_PI) * (double)kv.y) / a.box[1];
        const double kz = ((2.0 * EW_PI) * (double)kv.z) / a.box[2];
        const double k2 = (kx * kx + ky * ky) + kz * kz;
        const double A = exp(-(k2 / a.a4)) / k2;
        double* c = a.coef + 5 * (size_t)m;
        c[0] = A * C; c[1] = A * S; c[2] = kx; c[3] = ky; c[4] = kz;
        if (ENERGY) e = e + A * (C * C + S * S);
    }
}

__global__ __launch_bounds__(BLOCK) void ew_finalise_kernel(const EwaldArgs a) {
    double e = 0.0;
    finalise_body<false>(a, e);
}

__global__ __launch_bounds__(BLOCK) void ew_finalise_energy_kernel(const EwaldArgs a) {
    __shared__ Sum4Lds l;
    double e = 0.0;
    finalise_body<true>(a, e);
    sum4_store(l, a.rows, e, 0.0, 0.0, 0.0);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void ew_force_kernel(const EwaldArgs a) {
    const double* __restrict__ coef = a.coef;
    const int4* __restrict__ kvec = a.kvec;
    const double V = (a.box[0] * a.box[1]) * a.box[2];
    const double pref = (8.0 * (EW_PI * NB_COULOMB)) / V;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const double q = a.par[3 * (size_t)i];
        if (q == 0.0) continue;
        const Vec3 x = slot_position<PREC>(a.posq, a.posq_corr, i);
        const double sx = frac_coord(x.x, a.box[0]), sy = frac_coord(x.y, a.box[1]), sz = frac_coord(x.z, a.box[2]);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        for (int m = 0; m < a.m; m++) {
            const int4 kv = kvec[m];
            const double t = ((double)kv.x * sx + (double)kv.y * sy) + (double)kv.z * sz;
            double sn, cs;
            sincospi(2.0 * t, &sn, &cs);
            const double* c = coef + 5 * (size_t)m;
            const double wgt = c[0] * sn - c[1] * cs;
            fx = fx + c[2] * wgt;
            fy = fy + c[3] * wgt;
            fz = fz + c[4] * wgt;
        }
        const double pq = pref * q;
        Fixed3 sum;
        sum.add({pq * fx, pq * fy, pq * fz});
        add_to_planes(a.force, a.padded, i, sum);
    }
}

// A charged exception row (p1, p2), for the receiving slot at `role`:
//   d = x(receiver) - x(other), r2 = (dx^2 + dy^2) + dz^2, qq = K (q_p1 q_p2);  r2 == 0: no force, E = -(qq tsp);  otherwise
//   r = sqrt(r2), inv = 1 / r, ar = alpha r, ef = erf(ar), g = exp(-(ar ar)), dc = qq ((ef inv - tsp g) inv), c = -(dc inv), E = -(qq (ef inv))
template <int PREC, bool ENERGY>
__device__ __forceinline__ void exclusion_body(const EwaldExclusionArgs& a, double& e) {
    for_each_receiver(a.recv, a.force, a.padded, [&](const int slot, const int t, const int role, Fixed3& sum) {
        const int2 at = a.atoms[t];
        const Vec3 d = slot_position<PREC>(a.posq, a.posq_corr, slot) - slot_position<PREC>(a.posq, a.posq_corr, role == 0 ? at.y : at.x);
        const double r2 = dot(d, d);
        const double qq = NB_COULOMB * (a.par[3 * (size_t)at.x] * a.par[3 * (size_t)at.y]);
        if (r2 == 0.0) {
            if (ENERGY && role == 0) e = e + (-(qq * a.tsp));
            return;
        }
        const double rr = sqrt(r2), inv = 1.0 / rr;
        const double ar = a.alpha * rr;
        const double ef = erf(ar);
        const double g = exp(-(ar * ar));
        const double dc = qq * ((ef * inv - a.tsp * g) * inv);
        const double c = -(dc * inv);
        sum.add(c * d);
        if (ENERGY && role == 0) e = e + (-(qq * (ef * inv)));
    });
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void ew_exclusion_kernel(const EwaldExclusionArgs a) {
    double e = 0.0;
    exclusion_body<PREC, false>(a, e);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void ew_exclusion_energy_kernel(const EwaldExclusionArgs a) {
    __shared__ Sum4Lds l;
    double e = 0.0;
    exclusion_body<PREC, true>(a, e);
    sum4_store(l, a.rows, e, 0.0, 0.0, 0.0);
}

// One work-group, a thread its chunk of each kind of row (row_chunk)
__global__ __launch_bounds__(BLOCK) void ew_energy_sum_kernel(const double* __restrict__ rec_rows, const int n_rec, const double rec_scale, const double* __restrict__ exc_rows,
                                                              const int n_exc, const double* __restrict__ misc, const double e_self,
                                                              double* __restrict__ out) {
    __shared__ Sum4Lds l;
    int r0, r1;
    double s0 = 0.0, s3 = 0.0;
    row_chunk(n_rec, r0, r1);
    for (int r = r0; r < r1; r++) s0 = s0 + rec_rows[4 * (size_t)r];
    row_chunk(n_exc, r0, r1);
    for (int r = r0; r < r1; r++) s3 = s3 + exc_rows[4 * (size_t)r];
    sum4_put(l, s0, 0.0, 0.0, s3);
    __syncthreads();
    if (threadIdx.x < 4) {
        const double total = sum4_total(l);
        out[threadIdx.x] = threadIdx.x == 0 ? (rec_scale != 0.0 ? rec_scale : misc[1]) * total : (threadIdx.x == 1 ? e_self : (threadIdx.x == 2 ? misc[0] : total));
    }
}

hipError_t launch_ewald_exclusions(int precision, const EwaldExclusionArgs& a, hipStream_t s) {
    if (!a.atoms || !a.par || !receivers_ok(a.recv) || !a.posq || !a.force || a.padded < 1 || (precision == TGNH_PREC_MIXED && !a.posq_corr))
        return hipErrorInvalidValue;
    const int grid = index_grid(a.recv.n);
    if (a.rows) TGNH_LAUNCH_PREC(ew_exclusion_energy_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    else TGNH_LAUNCH_PREC(ew_exclusion_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ewald_reciprocal(int precision, const EwaldArgs& a, hipStream_t s, int stage) {
    if (a.n < 1 || a.m < 1 || a.m > EW_MAX_VECTORS || a.parts != ew_parts(a.n) || a.parts > 65535 || !a.kvec || !a.par || !a.posq ||
        (precision == TGNH_PREC_MIXED && !a.posq_corr) || !a.part_rows || !a.coef || !a.force || a.padded < a.n)
        return hipErrorInvalidValue;
    switch (stage) {
        case 0: TGNH_LAUNCH_PREC(ew_sum_kernel, precision, dim3(ew_sum_tiles(a.m), a.parts), dim3(BLOCK), 0, s, a); break;
        case 1:
            if (a.rows) TGNH_LAUNCH(ew_finalise_energy_kernel, index_grid(a.m), BLOCK, 0, s, a);
            else TGNH_LAUNCH(ew_finalise_kernel, index_grid(a.m), BLOCK, 0, s, a);
            break;
        case 2: TGNH_LAUNCH_PREC(ew_force_kernel, precision, dim3(index_grid(a.n)), dim3(BLOCK), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ewald_energy_sum(const double* rec_rows, int n_rec, double rec_scale, const double* exc_rows, int n_exc, const double* misc, double e_self,
                                   double* out, hipStream_t s) {
    if (!misc || !out || n_rec < 0 || n_exc < 0 || (n_rec > 0 && !rec_rows) || (n_exc > 0 && !exc_rows) || n_rec > EW_MAX_REC_ROWS || n_exc > INDEX_GRID_CAP)
        return hipErrorInvalidValue;
    TGNH_LAUNCH(ew_energy_sum_kernel, 1, BLOCK, 0, s, rec_rows, n_rec, rec_scale, exc_rows, n_exc, misc, e_self, out);
    return hipGetLastError();
}

}  // namespace tgnh
