// tgnh_constraints.hip -- the kernels behind tgnh_apply_constraints / tgnh_apply_velocity_constraints: every constraint cluster solved
// directly, one lane per cluster, with no data-dependent loop.  The library's own constraint stage for a host that has no OpenMM
// behind it (the glue keeps calling OpenMM's applyConstraints, Cu :363, :391); the harness' SHAKE (tgnh_harness.hip) stays beside it,
// for clusters this solver does not take.
//
// A cluster has the harness' canonical form (up to 4 atoms, distances for the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)), and at most
// three of its distances are constraints: K <= 3 multipliers.  The host has numbered them k = 0..K-1 in the canonical pair order
// (ConstraintArgs::pairs: first atom i_k, second atom j_k) and taken the inverse masses w from the descriptor's masses.  With
//   e_k(a) = +1 for a = i_k, -1 for a = j_k, 0 otherwise           r_k = x(i_k) - x(j_k), the bond vector BEFORE the move
//   c_kl   = sum over the atoms a of e_k(a) e_l(a) w(a)            (the inverse-mass coupling of two constraints: w_i + w_j for k = l)
// a multiplier lambda_k moves atom a by lambda_k e_k(a) w(a) r_k, so that the bond vectors AFTER the move are
//   s_k(lambda) = s_k(0) + sum_l lambda_l c_kl r_l.
// Positions stage (on posDelta): Newton's method on sigma_k(lambda) = |s_k|^2 - d_k^2 from lambda = 0, EXACTLY FOUR iterations, each one
// K x K solve (Cramer's rule) with the Jacobian J_kl = 2 (s_k . r_l) c_kl.  It converges quadratically: from displacements drawn
// without regard to the constraints (300 K, 1-2 fs) the violation is at fp64 rounding after four (DESIGN.md 3.12 has the table).
// Velocity stage (on velm): linear, ONE solve of sum_l (r_k . r_l) c_kl mu_l = r_k . (v(i_k) - v(j_k)); v(a) -= mu_k e_k(a) w(a) r_k.
// A cluster of K < 3 constraints is the same 3 x 3 system with the unused rows and columns set to the identity: the same
// instructions in every lane, and every array below is indexed by unrolled loop variables only (registers).
//
// Everything in fp64 in every precision, as in the harness (its comment in shake_kernel says why).  The gates are the harness' own,
// evaluated on the result: |sigma_k| <= 2 tol d_k^2, and |r_k . (v_i - v_j)| / r_k^2 <= tol; a result that fails one -- a NaN fails
// both -- sets status bit 1 and is stored all the same, as the harness stores what its last sweep left.  x, y, z of the cluster's atoms
// are written; w of posDelta and velm is stored back as read, and the masses never come from velm.
// No LDS, no atomic but the status word's, no inline assembly.
#include "tgnh_constraints.h"
#include "tgnh_device_math.h"

namespace tgnh {

// A cluster in registers: what both stages read before they differ
struct CnCluster {
    int at[4];
    double x[4][3];           // positions (mixed precision: posq + posq_correction), 0 for an unused atom
    double w[4];
    double e[3][4];           // e_k(a)
    double d2[3];
    bool on[3];               // constraint k exists
};

template <int PREC>
__device__ __forceinline__ void cn_load(const ConstraintArgs& a, int c, CnCluster& cl) {
    typedef typename Prec<PREC>::real4 real4;
    const real4* __restrict__ posq = reinterpret_cast<const real4*>(a.posq);
    const float4* __restrict__ pcorr = reinterpret_cast<const float4*>(a.posq_corr);
    const int4 at4 = a.atoms[c];
    const double4 w4 = a.invmass[c];
    const uint32_t pairs = a.pairs[c];
    cl.at[0] = at4.x; cl.at[1] = at4.y; cl.at[2] = at4.z; cl.at[3] = at4.w;
    cl.w[0] = w4.x; cl.w[1] = w4.y; cl.w[2] = w4.z; cl.w[3] = w4.w;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cl.x[k][0] = cl.x[k][1] = cl.x[k][2] = 0.0;
        if (cl.at[k] >= 0) {                                     // (the host checked at set time: a slot of the bound arrays)
            const real4 p = posq[cl.at[k]];
            cl.x[k][0] = p.x; cl.x[k][1] = p.y; cl.x[k][2] = p.z;
            if (PREC == TGNH_PREC_MIXED) { const float4 cc = pcorr[cl.at[k]]; cl.x[k][0] += (double)cc.x; cl.x[k][1] += (double)cc.y; cl.x[k][2] += (double)cc.z; }
        }
    }
    const int K = (int)((pairs >> 12) & 3u);
#pragma unroll
    for (int k = 0; k < CN_MAX_CONSTRAINTS; k++) {
        cl.on[k] = k < K;
        cl.d2[k] = cl.on[k] ? a.d2[(size_t)k * a.n + c] : 0.0;
        const int i = (int)((pairs >> (4 * k)) & 3u), j = (int)((pairs >> (4 * k + 2)) & 3u);
#pragma unroll
        for (int m = 0; m < 4; m++) cl.e[k][m] = !cl.on[k] ? 0.0 : (m == i ? 1.0 : (m == j ? -1.0 : 0.0));
    }
}

// v_k = sum_a e_k(a) u(a): the difference u(i_k) - u(j_k) with static indices (1 x, -1 x and exact zeros: the same bits as the difference)
__device__ __forceinline__ void cn_bond(const double (&e)[3][4], const double (&u)[4][3], double (&v)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) v[k][j] = e[k][0] * u[0][j] + e[k][1] * u[1][j] + e[k][2] * u[2][j] + e[k][3] * u[3][j];
}

__device__ __forceinline__ void cn_coupling(const CnCluster& cl, double (&c)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int l = 0; l < 3; l++)
            c[k][l] = cl.e[k][0] * cl.e[l][0] * cl.w[0] + cl.e[k][1] * cl.e[l][1] * cl.w[1] + cl.e[k][2] * cl.e[l][2] * cl.w[2] + cl.e[k][3] * cl.e[l][3] * cl.w[3];
}

__device__ __forceinline__ double cn_dot(const double (&p)[3], const double (&q)[3]) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; }

// A y = b by Cramer's rule (the adjugate); a singular A divides by zero and leaves non-finite numbers, which the gates refuse
__device__ __forceinline__ void cn_solve3(const double (&A)[3][3], const double (&b)[3], double (&y)[3]) {
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2], c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double c10 = A[0][2] * A[2][1] - A[0][1] * A[2][2], c11 = A[0][0] * A[2][2] - A[0][2] * A[2][0], c12 = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    const double c20 = A[0][1] * A[1][2] - A[0][2] * A[1][1], c21 = A[0][2] * A[1][0] - A[0][0] * A[1][2], c22 = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    const double inv = 1.0 / (A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02);
    y[0] = (c00 * b[0] + c10 * b[1] + c20 * b[2]) * inv;
    y[1] = (c01 * b[0] + c11 * b[1] + c21 * b[2]) * inv;
    y[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) * inv;
}

constexpr int CN_NEWTON_ITERATIONS = 4;

template <int PREC>
__global__ __launch_bounds__(BLOCK) void constrain_positions_kernel(const ConstraintArgs a) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    mixed4* __restrict__ pdelta = reinterpret_cast<mixed4*>(a.pos_delta);
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.n) return;
    CnCluster cl;
    cn_load<PREC>(a, c, cl);
    mixed4 keep[4];
    double q[4][3];                                              // the displacements
#pragma unroll
    for (int k = 0; k < 4; k++) {
        q[k][0] = q[k][1] = q[k][2] = 0.0;
        if (cl.at[k] >= 0) { keep[k] = pdelta[cl.at[k]]; q[k][0] = keep[k].x; q[k][1] = keep[k].y; q[k][2] = keep[k].z; }
    }
    double r[3][3], s0[3][3], cc[3][3];
    cn_bond(cl.e, cl.x, r);
    cn_bond(cl.e, q, s0);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) s0[k][j] += r[k][j];
    cn_coupling(cl, cc);
    double lam[3] = {0.0, 0.0, 0.0}, s[3][3], sigma[3];
    auto residual = [&]() {                                      // s_k(lambda) and sigma_k
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int j = 0; j < 3; j++) s[k][j] = s0[k][j] + (lam[0] * cc[k][0] * r[0][j] + lam[1] * cc[k][1] * r[1][j] + lam[2] * cc[k][2] * r[2][j]);
            sigma[k] = cn_dot(s[k], s[k]) - cl.d2[k];
        }
    };
#pragma unroll 1
    for (int it = 0; it < CN_NEWTON_ITERATIONS; it++) {
        residual();
        double J[3][3], b[3], dl[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int l = 0; l < 3; l++) J[k][l] = 2.0 * cn_dot(s[k], r[l]) * cc[k][l];
            if (!cl.on[k]) J[k][k] = 1.0;                        // (its row and column are zeros otherwise: e_k = 0)
            b[k] = -sigma[k];
        }
        cn_solve3(J, b, dl);
#pragma unroll
        for (int k = 0; k < 3; k++) lam[k] += dl[k];
    }
    residual();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double v = sigma[k] < 0 ? -sigma[k] : sigma[k];
        if (cl.on[k] && !(v <= 2.0 * a.tol * cl.d2[k])) ok = false;
    }
    if (!ok) atomicOr(a.status, 2u);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (cl.at[k] >= 0) {
            mixed4 o = keep[k];
#pragma unroll
            for (int j = 0; j < 3; j++)
                q[k][j] += (lam[0] * cl.e[0][k] * r[0][j] + lam[1] * cl.e[1][k] * r[1][j] + lam[2] * cl.e[2][k] * r[2][j]) * cl.w[k];
            o.x = (mixed)q[k][0]; o.y = (mixed)q[k][1]; o.z = (mixed)q[k][2];
            pdelta[cl.at[k]] = o;
        }
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void constrain_velocities_kernel(const ConstraintArgs a) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    mixed4* __restrict__ velm = reinterpret_cast<mixed4*>(a.velm);
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.n) return;
    CnCluster cl;
    cn_load<PREC>(a, c, cl);
    mixed4 keep[4];
    double q[4][3];                                              // the velocities
#pragma unroll
    for (int k = 0; k < 4; k++) {
        q[k][0] = q[k][1] = q[k][2] = 0.0;
        if (cl.at[k] >= 0) { keep[k] = velm[cl.at[k]]; q[k][0] = keep[k].x; q[k][1] = keep[k].y; q[k][2] = keep[k].z; }
    }
    double r[3][3], dv[3][3], cc[3][3], A[3][3], b[3], mu[3];
    cn_bond(cl.e, cl.x, r);
    cn_bond(cl.e, q, dv);
    cn_coupling(cl, cc);
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int l = 0; l < 3; l++) A[k][l] = cn_dot(r[k], r[l]) * cc[k][l];
        if (!cl.on[k]) A[k][k] = 1.0;
        b[k] = cn_dot(r[k], dv[k]);
    }
    cn_solve3(A, b, mu);
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            q[k][j] -= (mu[0] * cl.e[0][k] * r[0][j] + mu[1] * cl.e[1][k] * r[1][j] + mu[2] * cl.e[2][k] * r[2][j]) * cl.w[k];
    cn_bond(cl.e, q, dv);                                        // the gate looks at the velocities as they will be stored from
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double rate = cn_dot(r[k], dv[k]) / cn_dot(r[k], r[k]);
        if (cl.on[k] && !((rate < 0 ? -rate : rate) <= a.tol)) ok = false;
    }
    if (!ok) atomicOr(a.status, 2u);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (cl.at[k] >= 0) {
            mixed4 o = keep[k];
            o.x = (mixed)q[k][0]; o.y = (mixed)q[k][1]; o.z = (mixed)q[k][2];
            velm[cl.at[k]] = o;
        }
    }
}

static bool cn_args_ok(int precision, const ConstraintArgs& a) {
    if (a.n < 1 || !a.atoms || !a.invmass || !a.d2 || !a.pairs || !a.posq || !a.status) return false;
    return precision != TGNH_PREC_MIXED || a.posq_corr;
}

hipError_t launch_constrain_positions(int precision, const ConstraintArgs& a, hipStream_t s) {
    if (!cn_args_ok(precision, a) || !a.pos_delta) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(constrain_positions_kernel, precision, dim3(cn_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_constrain_velocities(int precision, const ConstraintArgs& a, hipStream_t s) {
    if (!cn_args_ok(precision, a) || !a.velm) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(constrain_velocities_kernel, precision, dim3(cn_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace tgnh
