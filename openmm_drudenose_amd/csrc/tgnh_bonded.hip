// tgnh_bonded.hip -- the kernels behind tgnh_compute_bonded_forces / tgnh_get_bonded_energy: OpenMM's HarmonicBondForce,
// HarmonicAngleForce and PeriodicTorsionForce for a host that has no OpenMM behind it (the glue keeps OpenMM's), beside the library's
// DrudeForce (tgnh_drude_force.hip).  The terms, as include/drude_tgnh.h writes them; x(i) is posq, + posq_correction in mixed precision.
//   bond (p1, p2; r0, k)           d = x(p2) - x(p1), r = |d|, c = (k (r - r0)) / r:                p1: +c d   p2: -c d      E = (1/2 k (r - r0)) (r - r0)
//   angle (p1, p2, p3; t0, k)      a = x(p1) - x(p2), b = x(p3) - x(p2), c = a x b, s = max(|c|, 1e-6), t = atan2(|c|, a . b), g = k (t - t0),
//                                  F1 = (g / ((a . a) s)) (c x a), F3 = (g / ((b . b) s)) (b x c):   p1: F1   p2: -(F1 + F3)   p3: F3   E = (1/2 g) (t - t0)
//   torsion (p1..p4; n, phi0, k)   v0 = x(p1) - x(p2), v1 = x(p3) - x(p2), v2 = x(p3) - x(p4), c0 = v0 x v1, c1 = v1 x v2, l = |v1|,
//                                  X = c0 . c1, Y = l (v0 . c1), hyp = sqrt(X^2 + Y^2), (C_1, S_1) = (X, Y) / hyp and the angle-addition
//                                  recurrence up to (C_n, S_n) = (cos n phi, sin n phi): no trigonometric call,
//                                  g = -(k n) (S_n cos phi0 - C_n sin phi0), F1 = (-g l / (c0 . c0)) c0, F4 = (g l / (c1 . c1)) c1,
//                                  s = ((v0 . v1) / (v1 . v1)) F1 - ((v2 . v1) / (v1 . v1)) F4:
//                                  p1: F1   p2: s - F1   p3: -s - F4   p4: F4                        E = k (1 + (C_n cos phi0 + S_n sin phi0))
// Everything in fp64 in every precision, every operation rounded on its own (no fused multiply-add: a test restates the bond shares in
// numpy and asks for the same bits); sqrt and the divisions are the IEEE ones.  Periodic images are not applied.
//
// FORM: tgnh_receiver_device.h's, one lane per RECEIVING slot over the tables the host inverted at set time (BondedArgs).  Per entry
// (term, role) a lane recomputes the term from its positions and forms its own share.
//
// ENERGY (the second instantiation, want_energy): the lane of a term's p1 counts it, once.  A thread adds its receivers in ascending
// order, the three kinds apart; the rest of the order is tgnh_rows_device.h's, and bonded_energy_sum_kernel -- one work-group -- adds
// the rows: the same bits from any handle over the same slots and the same tables.
//
// A bond of length 0 or a torsion whose c0 or c1 has length 0 divides by zero and stores what comes out.  A unit of its own so that
// the other units compile to what they compiled to before.
#include "tgnh_bonded.h"
#include "tgnh_receiver_device.h"
#include "tgnh_rows_device.h"

namespace tgnh {

#pragma clang fp contract(off)

namespace {
template <int PREC, bool ENERGY>
__device__ __forceinline__ void bond_term(const BondedArgs& a, const int t, const int role, Fixed3& sum, double& e_bond) {
    const int2 at = a.bond_atoms[t];
    const double2 par = a.bond_par[t];
    const Vec3 d = slot_position<PREC>(a.posq, a.posq_corr, at.y) - slot_position<PREC>(a.posq, a.posq_corr, at.x);
    const double r = sqrt(dot(d, d)), dr = r - par.x;
    const Vec3 f = ((par.y * dr) / r) * d;
    sum.add(role == BF_P1 ? f : neg(f));
    if (ENERGY && role == BF_P1) e_bond = e_bond + ((0.5 * par.y) * dr) * dr;
}

template <int PREC, bool ENERGY>
__device__ __forceinline__ void angle_term(const BondedArgs& a, const int t, const int role, Fixed3& sum, double& e_angle) {
    const int4 at = a.angle_atoms[t];
    const double2 par = a.angle_par[t];
    const Vec3 x2 = slot_position<PREC>(a.posq, a.posq_corr, at.y);
    const Vec3 va = slot_position<PREC>(a.posq, a.posq_corr, at.x) - x2, vb = slot_position<PREC>(a.posq, a.posq_corr, at.z) - x2;
    const Vec3 c = cross(va, vb);
    const double len = sqrt(dot(c, c)), s = fmax(len, 1e-6);
    const double dt = atan2(len, dot(va, vb)) - par.x, g = par.y * dt;
    Vec3 f1 = {0.0, 0.0, 0.0}, f3 = {0.0, 0.0, 0.0};
    if (role != BF_P3) f1 = (g / (dot(va, va) * s)) * cross(c, va);
    if (role != BF_P1) f3 = (g / (dot(vb, vb) * s)) * cross(vb, c);
    sum.add(role == BF_P1 ? f1 : (role == BF_P3 ? f3 : neg(f1 + f3)));
    if (ENERGY && role == BF_P1) e_angle = e_angle + (0.5 * g) * dt;
}

template <int PREC, bool ENERGY>
__device__ __forceinline__ void torsion_term(const BondedArgs& a, const int t, const int role, Fixed3& sum, double& e_torsion) {
    const int4 at = a.torsion_atoms[t];
    const int n = a.torsion_n[t];
    const double cos0 = a.torsion_par[t], sin0 = a.torsion_par[(size_t)a.n_torsions + t], k = a.torsion_par[2 * (size_t)a.n_torsions + t];
    const Vec3 x2 = slot_position<PREC>(a.posq, a.posq_corr, at.y), x3 = slot_position<PREC>(a.posq, a.posq_corr, at.z);
    const Vec3 v0 = slot_position<PREC>(a.posq, a.posq_corr, at.x) - x2, v1 = x3 - x2, v2 = x3 - slot_position<PREC>(a.posq, a.posq_corr, at.w);
    const Vec3 c0 = cross(v0, v1), c1 = cross(v1, v2);
    const double l2 = dot(v1, v1), l = sqrt(l2);
    const double X = dot(c0, c1), Y = l * dot(v0, c1), hyp = sqrt(X * X + Y * Y);
    const double cp = X / hyp, sp = Y / hyp;
    double C = cp, S = sp;
    for (int m = 1; m < n; m++) {                                // (C, S) = (cos m phi, sin m phi) -> m + 1
        const double c_next = C * cp - S * sp, s_next = S * cp + C * sp;
        C = c_next; S = s_next;
    }
    const double g = -(k * (double)n) * (S * cos0 - C * sin0);
    if (ENERGY && role == BF_P1) e_torsion = e_torsion + k * (1.0 + (C * cos0 + S * sin0));
    if (role == BF_P1) { sum.add(((-g * l) / dot(c0, c0)) * c0); return; }
    if (role == BF_P4) { sum.add(((g * l) / dot(c1, c1)) * c1); return; }
    const Vec3 f1 = ((-g * l) / dot(c0, c0)) * c0, f4 = ((g * l) / dot(c1, c1)) * c1;
    const Vec3 s = (dot(v0, v1) / l2) * f1 - (dot(v2, v1) / l2) * f4;
    sum.add(role == BF_P2 ? s - f1 : neg(s) - f4);
}

template <int PREC, bool ENERGY>
__device__ __forceinline__ void bonded_body(const BondedArgs& a, double& e_bond, double& e_angle, double& e_torsion) {
    const int first_angle = a.n_bonds, first_torsion = a.n_bonds + a.n_angles;
    // for_each_receiver's loop, written out (tgnh_receiver_device.h says why)
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.recv.n; it += (long long)gridDim.x * BLOCK) {
        const int r = (int)it;
        const int slot = a.recv.slot[r];
        const int e1 = a.recv.start[r + 1];
        Fixed3 sum;
        for (int e = a.recv.start[r]; e < e1; e++) {
            const int term = a.recv.term[e], role = a.recv.role[e];
            if (term < first_angle) bond_term<PREC, ENERGY>(a, term, role, sum, e_bond);
            else if (term < first_torsion) angle_term<PREC, ENERGY>(a, term - first_angle, role, sum, e_angle);
            else torsion_term<PREC, ENERGY>(a, term - first_torsion, role, sum, e_torsion);
        }
        add_to_planes(a.force, a.padded, slot, sum);
    }
}
}  // namespace

template <int PREC>
__global__ __launch_bounds__(BLOCK) void bonded_forces_kernel(const BondedArgs a) {
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    bonded_body<PREC, false>(a, e0, e1, e2);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void bonded_forces_energy_kernel(const BondedArgs a) {
    __shared__ Sum4Lds l;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    bonded_body<PREC, true>(a, e0, e1, e2);
    sum4_store(l, a.rows, e0, e1, e2, 0.0);
}

// rows [0, nrows)[4] -> out[4].  One work-group, a thread its chunk of the rows (row_chunk).
__global__ __launch_bounds__(BLOCK) void bonded_energy_sum_kernel(const double* __restrict__ rows, const int nrows, double* __restrict__ out) {
    __shared__ Sum4Lds l;
    int r0, r1;
    row_chunk(nrows, r0, r1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int r = r0; r < r1; r++) { s0 = s0 + rows[4 * (size_t)r]; s1 = s1 + rows[4 * (size_t)r + 1]; s2 = s2 + rows[4 * (size_t)r + 2]; }
    sum4_put(l, s0, s1, s2, 0.0);
    __syncthreads();
    if (threadIdx.x < 4) out[threadIdx.x] = sum4_total(l);
}

hipError_t launch_bonded_forces(int precision, const BondedArgs& a, hipStream_t s) {
    if (a.n_bonds < 0 || a.n_angles < 0 || a.n_torsions < 0 || (a.n_bonds > 0 && (!a.bond_atoms || !a.bond_par)) ||
        (a.n_angles > 0 && (!a.angle_atoms || !a.angle_par)) || (a.n_torsions > 0 && (!a.torsion_atoms || !a.torsion_n || !a.torsion_par)) ||
        !receivers_ok(a.recv) || !a.posq || !a.force || a.padded < 1 ||
        (precision == TGNH_PREC_MIXED && !a.posq_corr))
        return hipErrorInvalidValue;
    const int grid = bf_grid(a.recv.n);
    if (a.rows) TGNH_LAUNCH_PREC(bonded_forces_energy_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    else TGNH_LAUNCH_PREC(bonded_forces_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bonded_energy_sum(const double* rows, int nrows, double* out, hipStream_t s) {
    if (!rows || !out || nrows < 1 || nrows > INDEX_GRID_CAP) return hipErrorInvalidValue;
    TGNH_LAUNCH(bonded_energy_sum_kernel, 1, BLOCK, 0, s, rows, nrows, out);
    return hipGetLastError();
}

}  // namespace tgnh
