// tgnh_constraints.cpp -- the direct constraint solver's cluster table (checks, the rows in the kernels' form, sorted by smallest slot),
// tgnh_apply_constraints and tgnh_apply_velocity_constraints (tgnh_constraints.hip has the kernels; include/drude_tgnh.h the contract)
#include <numeric>

#include "tgnh_host.h"
#include "tgnh_constraints.h"

static const int CN_PA[6] = {0, 0, 0, 1, 1, 2}, CN_PB[6] = {1, 2, 3, 2, 3, 3};      // the canonical pair order

// what is wrong with the caller's arrays (TGNH_ERR_ARG), then what this solver does not take (TGNH_ERR_UNSUPPORTED): all before any device work
static tgnh_status clusters_check(const tgnh_context* c, int n, const int32_t* atoms, const double* dist) {
    const int N = c->d.num_particles;
    std::vector<int> owner((size_t)N, -1);
    for (int k = 0; k < n; k++) {
        const int32_t* at = atoms + 4 * (size_t)k;
        const double* d = dist + 6 * (size_t)k;
        const std::string who = "tgnh_set_constraint_clusters: cluster " + std::to_string(k);
        for (int m = 0; m < 4; m++) {
            if (at[m] < -1 || at[m] >= N) return fail(TGNH_ERR_ARG, who + ": atom index " + std::to_string(at[m]) + " out of range");
            if (at[m] < 0) continue;
            if (owner[at[m]] == k) return fail(TGNH_ERR_ARG, who + " lists atom " + std::to_string(at[m]) + " twice");
            if (owner[at[m]] >= 0)
                return fail(TGNH_ERR_ARG, who + " and cluster " + std::to_string(owner[at[m]]) + " share atom " + std::to_string(at[m]) + ": two lanes would write one slot");
            owner[at[m]] = k;
        }
        int K = 0;
        for (int p = 0; p < 6; p++) {
            if (!std::isfinite(d[p]) || d[p] < 0.0) return fail(TGNH_ERR_ARG, who + ": a distance is negative or not finite");
            if (d[p] == 0.0) continue;
            if (at[CN_PA[p]] < 0 || at[CN_PB[p]] < 0) return fail(TGNH_ERR_ARG, who + ": a constraint names an unused atom");
            K++;
        }
        if (K == 0) return fail(TGNH_ERR_ARG, who + " holds no constraint");
    }
    for (int k = 0; k < n; k++) {
        const int32_t* at = atoms + 4 * (size_t)k;
        const double* d = dist + 6 * (size_t)k;
        const std::string who = "tgnh_set_constraint_clusters: cluster " + std::to_string(k);
        int K = 0;
        for (int p = 0; p < 6; p++) {
            if (d[p] == 0.0) continue;
            K++;
            for (int a : {at[CN_PA[p]], at[CN_PB[p]]})
                if (c->topo.mass[a] == 0.0) return fail(TGNH_ERR_UNSUPPORTED, who + ": constrained atom " + std::to_string(a) + " has no mass");
        }
        if (K > CN_MAX_CONSTRAINTS)
            return fail(TGNH_ERR_UNSUPPORTED, who + " holds " + std::to_string(K) + " constraints; the direct solver takes at most " +
                                              std::to_string(CN_MAX_CONSTRAINTS) + ": leave it to an iterative solver");
    }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_constraint_clusters(tgnh_handle h, int n, const int32_t* atoms, const double* dist) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!atoms || !dist))) return fail(TGNH_ERR_ARG, "tgnh_set_constraint_clusters: bad cluster arrays");
    tgnh_status rc = clusters_check(h, n, atoms, dist); if (rc) return rc;
    if (h->host_only) { h->cons.count = n; return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    h->cons.drop();
    if (n == 0) return TGNH_OK;
    // rows by smallest slot index (ties cannot happen: no atom is shared), so that neighbouring lanes gather neighbouring lines
    std::vector<int> order((size_t)n), first((size_t)n);
    for (int k = 0; k < n; k++) {
        int lo = h->d.num_particles;
        for (int m = 0; m < 4; m++) if (atoms[4 * (size_t)k + m] >= 0) lo = std::min(lo, (int)atoms[4 * (size_t)k + m]);
        first[k] = lo;
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return first[x] < first[y]; });
    std::vector<int4> r_atoms((size_t)n);
    std::vector<double4> r_w((size_t)n);
    std::vector<double> r_d2(3 * (size_t)n, 0.0);
    std::vector<uint32_t> r_pairs((size_t)n);
    for (int row = 0; row < n; row++) {
        const int32_t* at = atoms + 4 * (size_t)order[row];
        const double* d = dist + 6 * (size_t)order[row];
        r_atoms[row] = make_int4(at[0], at[1], at[2], at[3]);
        double w[4];
        for (int m = 0; m < 4; m++) w[m] = at[m] >= 0 && h->topo.mass[at[m]] != 0.0 ? 1.0 / h->topo.mass[at[m]] : 0.0;
        r_w[row] = make_double4(w[0], w[1], w[2], w[3]);
        uint32_t pairs = 0, K = 0;
        for (int p = 0; p < 6; p++) {
            if (d[p] == 0.0) continue;
            r_d2[K * (size_t)n + row] = d[p] * d[p];
            pairs |= ((uint32_t)CN_PA[p] | (uint32_t)CN_PB[p] << 2) << (4 * K);
            K++;
        }
        r_pairs[row] = pairs | K << 12;
    }
    HIP_OK(h->cons.d_atoms.upload(r_atoms));
    HIP_OK(h->cons.d_invmass.upload(r_w));
    HIP_OK(h->cons.d_d2.upload(r_d2));
    HIP_OK(h->cons.d_pairs.upload(r_pairs));
    h->cons.count = n;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_num_constraint_clusters(tgnh_handle h, int* count) {
    CHECK_H(h);
    if (!count) return fail(TGNH_ERR_ARG, "null count");
    *count = h->cons.count;
    return TGNH_OK;
}

static ConstraintArgs constraint_args(tgnh_handle h, double tol) {
    ConstraintArgs a{};
    a.atoms = h->cons.d_atoms; a.invmass = h->cons.d_invmass; a.d2 = h->cons.d_d2; a.pairs = h->cons.d_pairs; a.n = h->cons.count;
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr; a.velm = h->bound.velm; a.pos_delta = h->bound.pos_delta;
    a.tol = tol; a.status = h->status.d_word;
    return a;
}

extern "C" tgnh_status tgnh_apply_constraints(tgnh_handle h, double tol, void* stream) {
    tgnh_status rc = feature_ready(h, "tgnh_apply_constraints", &tgnh_context::Bound::velm, false); if (rc) return rc;
    if (!h->bound.pos_delta) return fail(TGNH_ERR_STATE, "tgnh_apply_constraints: posDelta buffer not bound");
    if (h->cons.count == 0) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(launch_constrain_positions(h->d.precision, constraint_args(h, tol), (hipStream_t)stream));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_apply_velocity_constraints(tgnh_handle h, double tol, void* stream) {
    tgnh_status rc = feature_ready(h, "tgnh_apply_velocity_constraints", &tgnh_context::Bound::velm, false); if (rc) return rc;
    h->owed.ke_carry = false;                 // velocities are about to change behind the integrator, as in tgnh_harness_shake_velocities
    if (h->cons.count == 0) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    rc = velm_current(h, (hipStream_t)stream); if (rc) return rc;
    HIP_OK(launch_constrain_velocities(h->d.precision, constraint_args(h, tol), (hipStream_t)stream));
    return TGNH_OK;
}
