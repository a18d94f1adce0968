// tgnh_drude_force.cpp -- the library's DrudeForce table (checks, the spring constants formed in fp64, the shares by
// receiving slot), tgnh_compute_drude_force and tgnh_get_drude_energy (tgnh_drude_force.hip has the kernels; include/drude_tgnh.h
// the contract)
#include <climits>
#include <set>
#include <utility>

#include "tgnh_host.h"
#include "tgnh_drude_force.h"

static const double ONE_4PI_EPS0 = 138.935456;      // kJ nm / (mol e^2): OpenMM's, and the harness' water force's (tgnh_harness.hip)

namespace {
struct RowConstants { double k1, k2, k3; };
}

// what is wrong with the caller's arrays (TGNH_ERR_ARG), all before any device work; *k: the rows' constants where every row is fine
static tgnh_status drude_force_check(const tgnh_context* c, int n, const int32_t* particles, const double* params, int num_screened,
                                     const int32_t* screened, const double* thole, std::vector<RowConstants>* k) {
    const int N = c->d.num_particles;
    auto who = [](int r) { return "tgnh_set_drude_force: row " + std::to_string(r); };
    k->resize((size_t)n);
    for (int r = 0; r < n; r++) {
        const int32_t* at = particles + 5 * (size_t)r;
        const double q = params[4 * (size_t)r], alpha = params[4 * (size_t)r + 1], aniso12 = params[4 * (size_t)r + 2], aniso34 = params[4 * (size_t)r + 3];
        if (at[0] != c->topo.pair_drude[r] || at[1] != c->topo.pair_parent[r])
            return fail(TGNH_ERR_ARG, who(r) + " names (" + std::to_string(at[0]) + ", " + std::to_string(at[1]) + "), the descriptor's pair " + std::to_string(r) +
                                          " is (" + std::to_string(c->topo.pair_drude[r]) + ", " + std::to_string(c->topo.pair_parent[r]) + ")");
        for (int m = 2; m < 5; m++)
            if (at[m] != -1 && (at[m] < 0 || at[m] >= N)) return fail(TGNH_ERR_ARG, who(r) + ": index " + std::to_string(at[m]) + " out of range");
        if (at[2] != -1 && (at[2] == at[0] || at[2] == at[1])) return fail(TGNH_ERR_ARG, who(r) + ": p2 is p or p1");
        if ((at[3] == -1) != (at[4] == -1)) return fail(TGNH_ERR_ARG, who(r) + ": exactly one of p3 and p4 is -1");
        if (at[3] != -1 && at[3] == at[4]) return fail(TGNH_ERR_ARG, who(r) + ": p3 is p4");
        if (!std::isfinite(q)) return fail(TGNH_ERR_ARG, who(r) + ": the charge is not finite");
        if (!std::isfinite(alpha) || alpha <= 0.0) return fail(TGNH_ERR_ARG, who(r) + ": the polarizability is not finite or not positive");
        const bool has12 = at[2] != -1, has34 = at[3] != -1;
        if (has12 && (!std::isfinite(aniso12) || aniso12 <= 0.0)) return fail(TGNH_ERR_ARG, who(r) + ": aniso12 is not finite or not positive");
        if (has34 && (!std::isfinite(aniso34) || aniso34 <= 0.0)) return fail(TGNH_ERR_ARG, who(r) + ": aniso34 is not finite or not positive");
        const double a1 = has12 ? aniso12 : 1.0, a2 = has34 ? aniso34 : 1.0, a3 = 3.0 - a1 - a2;
        if (!(a3 > 0.0)) return fail(TGNH_ERR_ARG, who(r) + ": 3 - aniso12 - aniso34 is not positive");
        const double cq2 = ONE_4PI_EPS0 * q * q;
        RowConstants& out = (*k)[r];
        out.k3 = cq2 / (alpha * a3);
        out.k1 = has12 ? cq2 / (alpha * a1) - out.k3 : 0.0;
        out.k2 = has34 ? cq2 / (alpha * a2) - out.k3 : 0.0;
    }
    std::set<std::pair<int, int>> seen;
    for (int m = 0; m < num_screened; m++) {
        const int i = screened[2 * (size_t)m], j = screened[2 * (size_t)m + 1];
        const std::string pair = "tgnh_set_drude_force: screened pair " + std::to_string(m);
        if (i < 0 || i >= n || j < 0 || j >= n) return fail(TGNH_ERR_ARG, pair + ": row " + std::to_string(i < 0 || i >= n ? i : j) + " out of range");
        if (i == j) return fail(TGNH_ERR_ARG, pair + " names row " + std::to_string(i) + " twice");
        if (!seen.insert({std::min(i, j), std::max(i, j)}).second) return fail(TGNH_ERR_ARG, pair + ": rows (" + std::to_string(i) + ", " + std::to_string(j) + ") are listed twice");
        if (!std::isfinite(thole[m]) || thole[m] < 0.0) return fail(TGNH_ERR_ARG, pair + ": thole is negative or not finite");
    }
    if (5LL * n + 4LL * num_screened > INT_MAX) return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_drude_force: more terms than the inverted table's 32-bit offsets take");
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_drude_force(tgnh_handle h, int n, const int32_t* particles, const double* params, int num_screened,
                                            const int32_t* screened, const double* thole) {
    CHECK_H(h);
    if (n != 0 && n != h->d.num_pairs)
        return fail(TGNH_ERR_ARG, "tgnh_set_drude_force: " + std::to_string(n) + " rows, the descriptor has " + std::to_string(h->d.num_pairs) + " pairs (0 clears the table)");
    if (num_screened < 0 || (n == 0 && num_screened > 0) || (n > 0 && (!particles || !params)) || (num_screened > 0 && (!screened || !thole)))
        return fail(TGNH_ERR_ARG, "tgnh_set_drude_force: bad table arrays");
    std::vector<RowConstants> k;
    tgnh_status rc = drude_force_check(h, n, particles, params, num_screened, screened, thole, &k); if (rc) return rc;
    if (h->host_only) { h->dforce.rows = n; h->dforce.screened = num_screened; return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    if (n == 0) { h->dforce = tgnh_context::DrudeForce(); return TGNH_OK; }
    std::vector<int4> r_atoms((size_t)n);
    std::vector<int> r_p4((size_t)n);
    std::vector<double> r_k(3 * (size_t)n);
    std::vector<int2> r_pair((size_t)num_screened);
    std::vector<double2> r_par((size_t)num_screened);
    std::vector<Share> shares;                                   // pushed in term order
    for (int r = 0; r < n; r++) {
        const int32_t* at = particles + 5 * (size_t)r;
        r_atoms[r] = make_int4(at[0], at[1], at[2], at[3]);
        r_p4[r] = at[4];
        r_k[r] = k[r].k1; r_k[(size_t)n + r] = k[r].k2; r_k[2 * (size_t)n + r] = k[r].k3;
        for (int m = 0; m < 5; m++)
            if (at[m] != -1) shares.push_back({at[m], r, (unsigned char)m});
    }
    for (int m = 0; m < num_screened; m++) {
        const int i = screened[2 * (size_t)m], j = screened[2 * (size_t)m + 1];
        const double qi = params[4 * (size_t)i], qj = params[4 * (size_t)j], ai = params[4 * (size_t)i + 1], aj = params[4 * (size_t)j + 1];
        r_pair[m] = make_int2(i, j);
        r_par[m] = make_double2(thole[m] / std::pow(ai * aj, 1.0 / 6.0), ONE_4PI_EPS0 * qi * qj);
        const int site[4] = {particles[5 * (size_t)i], particles[5 * (size_t)i + 1], particles[5 * (size_t)j], particles[5 * (size_t)j + 1]};
        for (int role = 0; role < 4; role++) shares.push_back({site[role], n + m, (unsigned char)role});
    }
    tgnh_context::DrudeForce f;                                  // built aside: an upload that fails leaves the table in force as it was
    HIP_OK(f.d_atoms.upload(r_atoms));
    HIP_OK(f.d_p4.upload(r_p4));
    HIP_OK(f.d_k.upload(r_k));
    HIP_OK(f.d_pair_rows.upload(r_pair));
    HIP_OK(f.d_pair_par.upload(r_par));
    HIP_OK(f.recv.upload(invert_shares(std::move(shares))));
    HIP_OK(f.d_energy.alloc(4 * ((size_t)df_grid(f.recv.n) + 1), true));     // the energy rows now: the launch may be recorded into a graph
    f.rows = n; f.screened = num_screened;
    h->dforce = std::move(f);                                    // (the old table's buffers are released here)
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_num_drude_force_terms(tgnh_handle h, int* rows, int* screened_pairs) {
    CHECK_H(h);
    if (!rows || !screened_pairs) return fail(TGNH_ERR_ARG, "null count");
    *rows = h->dforce.rows;
    *screened_pairs = h->dforce.screened;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_compute_drude_force(tgnh_handle h, void* force, int want_energy, void* stream) {
    tgnh_status rc = feature_ready(h, "tgnh_compute_drude_force", &tgnh_context::Bound::posq, true); if (rc) return rc;
    if (!force) return fail(TGNH_ERR_STATE, "tgnh_compute_drude_force: no force buffer");
    const tgnh_context::DrudeForce& f = h->dforce;
    if (f.rows == 0) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    DrudeForceArgs a{};
    a.atoms = f.d_atoms; a.p4 = f.d_p4; a.k = f.d_k; a.pair_rows = f.d_pair_rows; a.pair_par = f.d_pair_par;
    a.n_rows = f.rows; a.n_screened = f.screened;
    a.recv = f.recv.view();
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr;
    a.force = static_cast<long long*>(force); a.padded = h->d.padded_num_particles;
    a.rows = want_energy ? f.d_energy.get() : nullptr;
    Timed t(h, (hipStream_t)stream, KID_OTHER);
    HIP_OK(launch_drude_force(h->d.precision, a, (hipStream_t)stream));
    // (a launch recorded into a stream capture has not run: it fills the rows when the graph is replayed, and does not count here)
    if (want_energy && !stream_capturing((hipStream_t)stream)) h->dforce.energy_launched = true;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_drude_energy(tgnh_handle h, void* stream, double out[2]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    tgnh_status rc = feature_ready(h, "tgnh_get_drude_energy", &tgnh_context::Bound::posq, true); if (rc) return rc;
    const tgnh_context::DrudeForce& f = h->dforce;
    if (!f.energy_launched) return fail(TGNH_ERR_STATE, "tgnh_get_drude_energy: no tgnh_compute_drude_force with want_energy since the table was set");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int grid = df_grid(f.recv.n);
    double* totals = f.d_energy.get() + 4 * (size_t)grid;
    HIP_OK(launch_drude_energy_sum(f.d_energy, grid, totals, s));
    double got[4];
    rc = fetch_totals(h, totals, s, got); if (rc) return rc;
    out[0] = got[0]; out[1] = got[1];
    return TGNH_OK;
}
