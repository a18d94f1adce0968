// tgnh_drude_force.hip -- the kernels behind tgnh_compute_drude_force / tgnh_get_drude_energy: the library's own DrudeForce for a host
// that has no OpenMM behind it (the glue keeps OpenMM's); the harness' force_kernel and water_force_kernel (tgnh_harness.hip) stay
// beside it.  The terms are OpenMM's, as include/drude_tgnh.h writes them; x(i) is posq, + posq_correction in mixed precision.
//   per row (p, p1, p2, p3, p4), delta = x(p) - x(p1):
//     isotropic        t = k3 delta:                                                     p: -t    p1: +t                     E = 1/2 k3 |delta|^2
//     first axis       d = x(p1) - x(p2), e = d / |d|, s = e . delta,
//                      f1 = (k1 s) e, f2 = (k1 s / |d|)(delta - s e):                    p: -f1   p1: f1 - f2   p2: f2       E = 1/2 k1 s^2
//     second axis      d = x(p3) - x(p4), the same with k2:                              p: -f1   p1: f1   p3: -f2   p4: f2  E = 1/2 k2 s^2
//   per screened pair of rows (i, j), the four site pairs (first in {p_i, p1_i}, second in {p_j, p1_j}), sigma = +1 for Drude-Drude and
//   parent-parent, -1 for the mixed ones, delta = x(first) - x(second), r = |delta|, u = a r, S = 1 - (1 + u/2) exp(-u):
//     v = (sigma K (S / r - 1/2 (1 + u) exp(-u) a) / r^2) delta:                         first: +v   second: -v              E = sigma K S / r
// Everything in fp64 in every precision, every operation rounded on its own (no fused multiply-add: a test restates the isotropic
// shares in numpy and asks for the same bits); sqrt, exp and the divisions are the IEEE ones.
//
// FORM: tgnh_receiver_device.h's, one lane per RECEIVING slot over the table the host inverted at set time (DrudeForceArgs).  Per
// entry (term, role) a lane recomputes the term from the positions its role needs and forms its own share of every spring or site
// pair of that term.
//
// ENERGY (the second instantiation, want_energy): the lane of a row's p counts that row's springs, the lane of row i's p a screened
// pair's four site pairs (it forms the two pairs of p1_i for that alone); a term is counted once.  A thread adds its receivers in
// ascending order, springs and screened pairs apart; the rest of the order is tgnh_rows_device.h's, and drude_energy_sum_kernel -- one
// work-group -- adds the rows: the same bits from any handle over the same slots and the same table.
//
// A pair at r = 0 or an axis of length 0 divides by zero and stores what comes out.  A unit of its own so that the step kernels'
// units compile to what they compiled to before.
#include "tgnh_drude_force.h"
#include "tgnh_receiver_device.h"
#include "tgnh_rows_device.h"

namespace tgnh {

#pragma clang fp contract(off)

// one anisotropic spring along d: f1 = (k s) e, f2 = (k s / |d|)(delta - s e), E = 1/2 k s^2
struct AxisTerm { Vec3 f1, f2; double energy; };
__device__ __forceinline__ AxisTerm axis_term(const double k, const Vec3 d, const Vec3 delta) {
    const double len = sqrt(dot(d, d));
    const Vec3 e = {d.x / len, d.y / len, d.z / len};
    const double s = dot(e, delta), ks = k * s;
    AxisTerm t;
    t.f1 = ks * e;
    t.f2 = (ks / len) * (delta - s * e);
    t.energy = (0.5 * ks) * s;
    return t;
}

// one screened site pair, delta = x(first) - x(second), sk = sigma K: the share of `first` (the second's is its negative) and E
struct ScreenedTerm { Vec3 v; double energy; };
__device__ __forceinline__ ScreenedTerm screened_term(const double a, const double sk, const Vec3 delta) {
    const double r2 = dot(delta, delta), r = sqrt(r2);
    const double u = a * r, ex = exp(-u);
    const double S = 1.0 - (1.0 + 0.5 * u) * ex;
    const double c = (sk * (S / r - ((0.5 * (1.0 + u)) * ex) * a)) / r2;
    ScreenedTerm t;
    t.v = c * delta;
    t.energy = (sk * S) / r;
    return t;
}

template <int PREC, bool ENERGY>
__device__ __forceinline__ void drude_force_body(const DrudeForceArgs& a, double& e_spring, double& e_screened) {
    // for_each_receiver's loop, written out (tgnh_receiver_device.h says why)
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.recv.n; it += (long long)gridDim.x * BLOCK) {
        const int r = (int)it;
        const int slot = a.recv.slot[r];
        const int e1 = a.recv.start[r + 1];
        Fixed3 sum;
        for (int e = a.recv.start[r]; e < e1; e++) {
            const int term = a.recv.term[e], role = a.recv.role[e];
            if (term < a.n_rows) {
                const int4 at = a.atoms[term];
                const Vec3 xp = slot_position<PREC>(a.posq, a.posq_corr, at.x), x1 = slot_position<PREC>(a.posq, a.posq_corr, at.y);
                const Vec3 delta = xp - x1;
                double energy = 0.0;
                if (role <= DF_P1) {
                    const double k3 = a.k[2 * (size_t)a.n_rows + term];
                    const Vec3 t = k3 * delta;
                    sum.add(role == DF_P ? neg(t) : t);
                    if (ENERGY) energy = (0.5 * k3) * dot(delta, delta);
                }
                if (at.z >= 0 && role <= DF_P2) {
                    const AxisTerm t = axis_term(a.k[term], x1 - slot_position<PREC>(a.posq, a.posq_corr, at.z), delta);
                    sum.add(role == DF_P ? neg(t.f1) : (role == DF_P1 ? t.f1 - t.f2 : t.f2));
                    if (ENERGY) energy = energy + t.energy;
                }
                if (at.w >= 0 && role != DF_P2) {
                    const Vec3 d = slot_position<PREC>(a.posq, a.posq_corr, at.w) - slot_position<PREC>(a.posq, a.posq_corr, a.p4[term]);
                    const AxisTerm t = axis_term(a.k[(size_t)a.n_rows + term], d, delta);
                    sum.add(role == DF_P ? neg(t.f1) : (role == DF_P1 ? t.f1 : (role == DF_P3 ? neg(t.f2) : t.f2)));
                    if (ENERGY) energy = energy + t.energy;
                }
                if (ENERGY && role == DF_P) e_spring = e_spring + energy;
            } else {
                const int m = term - a.n_rows;
                const int2 ij = a.pair_rows[m];
                const double2 par = a.pair_par[m];
                const int4 ai = a.atoms[ij.x], aj = a.atoms[ij.y];
                // the two sites of the other row, Drude first; this lane's site is `first` of its two site pairs when it belongs to row i
                const bool mine_i = role <= DF_PARENT_I, drude = (role & 1) == 0;
                const Vec3 me = slot_position<PREC>(a.posq, a.posq_corr, slot);
                const Vec3 od = slot_position<PREC>(a.posq, a.posq_corr, mine_i ? aj.x : ai.x), op = slot_position<PREC>(a.posq, a.posq_corr, mine_i ? aj.y : ai.y);
                const ScreenedTerm td = screened_term(par.x, drude ? par.y : -par.y, mine_i ? me - od : od - me);
                const ScreenedTerm tp = screened_term(par.x, drude ? -par.y : par.y, mine_i ? me - op : op - me);
                // (in the order of the site pairs as the header lists them: for a site of row j the Drude of row i comes first too)
                sum.add(mine_i ? td.v : neg(td.v));
                sum.add(mine_i ? tp.v : neg(tp.v));
                if (ENERGY && role == DF_DRUDE_I) {
                    const Vec3 xq = slot_position<PREC>(a.posq, a.posq_corr, ai.y);
                    const ScreenedTerm ud = screened_term(par.x, -par.y, xq - od), up = screened_term(par.x, par.y, xq - op);
                    e_screened = e_screened + (((td.energy + tp.energy) + ud.energy) + up.energy);
                }
            }
        }
        add_to_planes(a.force, a.padded, slot, sum);
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void drude_force_kernel(const DrudeForceArgs a) {
    double e0 = 0.0, e1 = 0.0;
    drude_force_body<PREC, false>(a, e0, e1);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void drude_force_energy_kernel(const DrudeForceArgs a) {
    __shared__ Sum4Lds l;
    double e0 = 0.0, e1 = 0.0;
    drude_force_body<PREC, true>(a, e0, e1);
    sum4_store(l, a.rows, e0, e1, 0.0, 0.0);
}

// rows [0, nrows)[4] -> out[4].  One work-group, a thread its chunk of the rows (row_chunk).
__global__ __launch_bounds__(BLOCK) void drude_energy_sum_kernel(const double* __restrict__ rows, const int nrows, double* __restrict__ out) {
    __shared__ Sum4Lds l;
    int r0, r1;
    row_chunk(nrows, r0, r1);
    double s0 = 0.0, s1 = 0.0;
    for (int r = r0; r < r1; r++) { s0 = s0 + rows[4 * (size_t)r]; s1 = s1 + rows[4 * (size_t)r + 1]; }
    sum4_put(l, s0, s1, 0.0, 0.0);
    __syncthreads();
    if (threadIdx.x < 4) out[threadIdx.x] = sum4_total(l);
}

hipError_t launch_drude_force(int precision, const DrudeForceArgs& a, hipStream_t s) {
    if (a.n_rows < 1 || a.n_screened < 0 || !a.atoms || !a.p4 || !a.k || (a.n_screened > 0 && (!a.pair_rows || !a.pair_par)) ||
        !receivers_ok(a.recv) || !a.posq || !a.force || a.padded < 1 ||
        (precision == TGNH_PREC_MIXED && !a.posq_corr))
        return hipErrorInvalidValue;
    const int grid = df_grid(a.recv.n);
    if (a.rows) TGNH_LAUNCH_PREC(drude_force_energy_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    else TGNH_LAUNCH_PREC(drude_force_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_drude_energy_sum(const double* rows, int nrows, double* out, hipStream_t s) {
    if (!rows || !out || nrows < 1 || nrows > INDEX_GRID_CAP) return hipErrorInvalidValue;
    TGNH_LAUNCH(drude_energy_sum_kernel, 1, BLOCK, 0, s, rows, nrows, out);
    return hipGetLastError();
}

}  // namespace tgnh
