// tgnh_virtual_sites.cpp -- the library's virtual-site table (checks, the rows in the kernels' form sorted by site slot, its
// shares by receiving slot), tgnh_compute_virtual_sites and tgnh_distribute_virtual_site_forces (tgnh_virtual_sites.hip has the
// kernels; include/drude_tgnh.h the contract)
#include <climits>
#include <numeric>

#include "tgnh_host.h"
#include "tgnh_virtual_sites.h"

static_assert(VS_TWO_AVERAGE == TGNH_SITE_TWO_AVERAGE && VS_THREE_AVERAGE == TGNH_SITE_THREE_AVERAGE && VS_OUT_OF_PLANE == TGNH_SITE_OUT_OF_PLANE &&
              VS_LOCAL_COORDINATES == TGNH_SITE_LOCAL_COORDINATES && VS_PARAMS == TGNH_SITE_PARAMS, "the header's site kinds are the kernels'");

static int parents_of(int kind) { return kind == VS_TWO_AVERAGE ? 2 : 3; }

// what is wrong with the caller's arrays (TGNH_ERR_ARG), then what this stage does not take (TGNH_ERR_UNSUPPORTED): all before any device work
static tgnh_status sites_check(const tgnh_context* c, int n, const int32_t* kind, const int32_t* atoms, const double* params) {
    const int N = c->d.num_particles;
    std::vector<unsigned char> is_site((size_t)N, 0);
    auto who = [](int k) { return "tgnh_set_virtual_sites: site " + std::to_string(k); };
    for (int k = 0; k < n; k++) {
        const int32_t* at = atoms + 4 * (size_t)k;
        const double* p = params + VS_PARAMS * (size_t)k;
        if (kind[k] < 0 || kind[k] >= VS_KINDS) return fail(TGNH_ERR_ARG, who(k) + ": unknown kind " + std::to_string(kind[k]));
        const int np = parents_of(kind[k]);
        if (np == 3 && at[3] == -1) return fail(TGNH_ERR_ARG, who(k) + ": p3 = -1, and its kind needs three parents");
        for (int m = 0; m < 4; m++) {
            if (m == 3 && np == 2 && at[3] == -1) continue;
            if (at[m] < 0 || at[m] >= N) return fail(TGNH_ERR_ARG, who(k) + ": index " + std::to_string(at[m]) + " out of range");
        }
        if (is_site[at[0]]) return fail(TGNH_ERR_ARG, who(k) + ": slot " + std::to_string(at[0]) + " is listed as a site twice");
        is_site[at[0]] = 1;
        for (int m = 1; m <= np; m++)
            for (int q = m + 1; q <= np; q++)
                if (at[m] == at[q]) return fail(TGNH_ERR_ARG, who(k) + " lists parent " + std::to_string(at[m]) + " twice");
        for (int j = 0; j < VS_PARAMS_USED[kind[k]]; j++)
            if (!std::isfinite(p[j])) return fail(TGNH_ERR_ARG, who(k) + ": a parameter is not finite");
        if (kind[k] == VS_LOCAL_COORDINATES) {               // OpenMM's own gate on the weights of a LocalCoordinatesSite
            const double so = p[0] + p[1] + p[2], sx = p[3] + p[4] + p[5], sy = p[6] + p[7] + p[8];
            if (std::fabs(so - 1.0) > 1e-6) return fail(TGNH_ERR_ARG, who(k) + ": the origin weights do not sum to 1");
            if (std::fabs(sx) > 1e-6 || std::fabs(sy) > 1e-6) return fail(TGNH_ERR_ARG, who(k) + ": the x or y weights do not sum to 0");
        }
    }
    for (int k = 0; k < n; k++)
        for (int m = 1; m <= parents_of(kind[k]); m++)
            if (is_site[atoms[4 * (size_t)k + m]])
                return fail(TGNH_ERR_ARG, who(k) + ": parent " + std::to_string(atoms[4 * (size_t)k + m]) + " is itself a site");
    std::vector<unsigned char> in_pair((size_t)N, 0);
    for (int i : c->topo.pair_drude) in_pair[i] = 1;
    for (int i : c->topo.pair_parent) in_pair[i] = 1;
    for (int k = 0; k < n; k++) {
        const int s = atoms[4 * (size_t)k];
        if (in_pair[s]) return fail(TGNH_ERR_UNSUPPORTED, who(k) + ": slot " + std::to_string(s) + " is a member of a Drude pair");      // (first: such a slot has a mass too)
        if (c->topo.mass[s] != 0.0) return fail(TGNH_ERR_UNSUPPORTED, who(k) + ": slot " + std::to_string(s) + " has a mass in the descriptor: a virtual site has none");
    }
    if (3 * (long long)n > INT_MAX) return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_virtual_sites: more sites than the inverted table's 32-bit offsets take");
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_virtual_sites(tgnh_handle h, int n, const int32_t* kind, const int32_t* atoms, const double* params) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!kind || !atoms || !params))) return fail(TGNH_ERR_ARG, "tgnh_set_virtual_sites: bad site arrays");
    tgnh_status rc = sites_check(h, n, kind, atoms, params); if (rc) return rc;
    if (h->host_only) { h->vsites.count = n; return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    if (n == 0) { h->vsites = tgnh_context::VirtualSites(); return TGNH_OK; }
    // rows by site slot (no slot is a site twice: no ties), so that neighbouring lanes write neighbouring lines
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return atoms[4 * (size_t)x] < atoms[4 * (size_t)y]; });
    std::vector<int4> r_atoms((size_t)n);
    std::vector<int> r_kind((size_t)n);
    std::vector<double> r_params(VS_PARAMS * (size_t)n, 0.0);
    std::vector<Share> shares;                                   // pushed in row order
    for (int row = 0; row < n; row++) {
        const int32_t* at = atoms + 4 * (size_t)order[row];
        const int k = kind[order[row]], np = parents_of(k);
        r_atoms[row] = make_int4(at[0], at[1], at[2], np == 3 ? at[3] : -1);
        r_kind[row] = k;
        for (int j = 0; j < VS_PARAMS_USED[k]; j++) r_params[j * (size_t)n + row] = params[VS_PARAMS * (size_t)order[row] + j];
        for (int m = 0; m < np; m++) shares.push_back({at[1 + m], row, (unsigned char)m});
    }
    tgnh_context::VirtualSites f;                                // built aside: an upload that fails leaves the table in force as it was
    HIP_OK(f.d_atoms.upload(r_atoms));
    HIP_OK(f.d_kind.upload(r_kind));
    HIP_OK(f.d_params.upload(r_params));
    HIP_OK(f.recv.upload(invert_shares(std::move(shares))));
    f.count = n;
    h->vsites = std::move(f);                                    // (the old table's buffers are released here)
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_num_virtual_sites(tgnh_handle h, int* count) {
    CHECK_H(h);
    if (!count) return fail(TGNH_ERR_ARG, "null count");
    *count = h->vsites.count;
    return TGNH_OK;
}

static SiteTable site_table(tgnh_handle h) {
    SiteTable t{};
    t.atoms = h->vsites.d_atoms; t.kind = h->vsites.d_kind; t.params = h->vsites.d_params; t.n = h->vsites.count;
    return t;
}

extern "C" tgnh_status tgnh_compute_virtual_sites(tgnh_handle h, void* stream) {
    tgnh_status rc = feature_ready(h, "tgnh_compute_virtual_sites", &tgnh_context::Bound::posq, false); if (rc) return rc;
    if (h->vsites.count == 0) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    SitePlaceArgs a{};
    a.t = site_table(h); a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr;
    HIP_OK(launch_place_sites(h->d.precision, a, (hipStream_t)stream));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_distribute_virtual_site_forces(tgnh_handle h, void* force, void* stream) {
    tgnh_status rc = feature_ready(h, "tgnh_distribute_virtual_site_forces", &tgnh_context::Bound::posq, false); if (rc) return rc;
    if (!force) return fail(TGNH_ERR_STATE, "tgnh_distribute_virtual_site_forces: no force buffer");
    if (h->vsites.count == 0) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    SiteSpreadArgs a{};
    a.t = site_table(h);
    a.recv = h->vsites.recv.view();
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr;
    a.force = static_cast<long long*>(force); a.padded = h->d.padded_num_particles;
    HIP_OK(launch_spread_site_forces(h->d.precision, a, (hipStream_t)stream));
    return TGNH_OK;
}
