// tgnh_ewald.cpp -- Ewald summation on top of the library's NonbondedForce: tgnh_set_nonbonded_ewald (the checks -- the part tgnh_set_nonbonded_pme shares written once --, the table of
// reciprocal vectors, the set-time constants, the receiver table of the exclusion correction, every buffer the compute call will
// need), tgnh_get_nonbonded_ewald and tgnh_get_ewald_energy.  tgnh_compute_nonbonded_force (tgnh_nonbonded.cpp) makes the launches;
// tgnh_ewald.hip has the kernels; include/drude_tgnh.h the contract.
#include "tgnh_host.h"
#include "tgnh_pme.h"

#pragma clang fp contract(off)      // tsp, a4, the self energy and bg_num are part of the contract: every operation rounded on its own

// What the two forms of the setting share (tgnh_set_nonbonded_pme is tgnh_pme.cpp's), written once.
// The head: the refusal inside a capture, the clearing call, the table that must be in force.  *done: the call has been answered
tgnh_status ewald_set_begin(tgnh_handle h, const char* me, bool clear, bool* done) {
    tgnh_context::Nonbonded& f = h->nonbonded;
    *done = true;
    if (!h->host_only && stream_capturing(f.last_stream))
        return fail(TGNH_ERR_STATE, std::string(me) + "the stream of the last tgnh_compute_nonbonded_force is capturing: the uploads here are synchronous, "
                                                      "call it outside the capture");
    if (clear) {
        if (!h->host_only) HIP_OK(hipSetDevice(h->device));
        h->ewald = tgnh_context::Ewald();
        f.energy_launched = false;                               // (slot 0 of the energy changes its meaning)
        return TGNH_OK;
    }
    if (f.particles == 0) return fail(TGNH_ERR_STATE, std::string(me) + "no nonbonded table is set: tgnh_set_nonbonded_force comes first");
    *done = false;
    return TGNH_OK;
}

// the constants of alpha, on any handle
void ewald_set_constants(tgnh_context::Ewald& e, double alpha) {
    e.on = true;
    e.alpha = alpha;
    e.tsp = (2.0 * alpha) / std::sqrt(EW_PI);
    e.a4 = 4.0 * (alpha * alpha);
}

// on a handle with a device, into a setting built aside: E_self, bgn, the exclusion correction's rows and their receiver table,
// where the energies land
tgnh_status ewald_set_shared(tgnh_handle h, tgnh_context::Ewald& e) {
    const tgnh_context::Nonbonded& f = h->nonbonded;
    const int n = f.particles;
    const double alpha = e.alpha, root_pi = std::sqrt(EW_PI);
    double q2 = 0.0, Q = 0.0;
    for (int i = 0; i < n; i++) { q2 = q2 + f.h_charge[i] * f.h_charge[i]; Q = Q + f.h_charge[i]; }      // slot order
    e.e_self = -((NB_COULOMB * (alpha / root_pi)) * q2);
    e.bg_num = ((EW_PI * NB_COULOMB) * (Q * Q)) / (2.0 * (alpha * alpha));
    HIP_OK(hipSetDevice(h->device));
    // the exclusion correction: every exception row, evaluated or not, whose particles' table charges have a non-zero product
    std::vector<int2> atoms; std::vector<Share> shares;
    for (const int2& at : f.h_exc) {
        if (f.h_charge[at.x] * f.h_charge[at.y] == 0.0) continue;
        const int t = (int)atoms.size();
        atoms.push_back(at);
        shares.push_back({at.x, t, 0}); shares.push_back({at.y, t, 1});
    }
    e.corrected = (int)atoms.size();
    if (e.corrected) {
        HIP_OK(e.d_exc_atoms.upload(atoms));
        HIP_OK(e.recv.upload(invert_shares(std::move(shares))));
        HIP_OK(e.d_exc_rows.alloc(4 * (size_t)index_grid(e.recv.n), true));
    }
    HIP_OK(e.d_misc.alloc(2, true));
    HIP_OK(e.d_totals.alloc(4, true));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_nonbonded_ewald(tgnh_handle h, const tgnh_ewald_desc* d) {
    CHECK_H(h);
    const char* me = "tgnh_set_nonbonded_ewald: ";
    tgnh_context::Nonbonded& f = h->nonbonded;
    bool done;
    tgnh_status rc = ewald_set_begin(h, me, d == nullptr, &done);
    if (rc || done) return rc;
    if (d->struct_size != sizeof(tgnh_ewald_desc))
        return fail(TGNH_ERR_ARG, std::string(me) + "struct_size " + std::to_string(d->struct_size) + " is not sizeof(tgnh_ewald_desc)");
    if (!std::isfinite(d->alpha) || d->alpha <= 0.0) return fail(TGNH_ERR_ARG, std::string(me) + "alpha is not finite or not positive");
    for (int k = 0; k < 3; k++)
        if (d->kmax[k] < 0 || d->kmax[k] > EW_MAX_KMAX)
            return fail(TGNH_ERR_ARG, std::string(me) + "kmax[" + std::to_string(k) + "] = " + std::to_string(d->kmax[k]) + " is not in [0, 255]");
    const long long M = ew_num_vectors(d->kmax);
    if (M > EW_MAX_VECTORS)
        return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + std::to_string(M) + " reciprocal vectors: more than 2^20 (the explicit sum is not built for that: "
                                                            "tgnh_set_nonbonded_pme is)");

    tgnh_context::Ewald e;                                       // built aside: a refusal or an upload that fails leaves what was in force
    ewald_set_constants(e, d->alpha);
    for (int k = 0; k < 3; k++) e.kmax[k] = d->kmax[k];
    e.vectors = (int)M; e.parts = ew_parts(f.particles);
    if (e.parts > 65535) return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "more than 65535 parts of slots");
    if (h->host_only) { h->ewald = std::move(e); f.energy_launched = false; return TGNH_OK; }
    rc = ewald_set_shared(h, e); if (rc) return rc;
    // the half space in the order nx, then ny, then nz, ascending: the first non-zero component is positive
    std::vector<int4> kvec;
    kvec.reserve((size_t)M);
    for (int nx = 0; nx <= e.kmax[0]; nx++)
        for (int ny = nx == 0 ? 0 : -e.kmax[1]; ny <= e.kmax[1]; ny++)
            for (int nz = (nx == 0 && ny == 0) ? 1 : -e.kmax[2]; nz <= e.kmax[2]; nz++) kvec.push_back(make_int4(nx, ny, nz, 0));
    if ((long long)kvec.size() != M) return fail(TGNH_ERR_STATE, std::string(me) + "internal: the table of vectors does not have M rows");
    if (M > 0) {
        HIP_OK(e.d_kvec.upload(kvec));
        HIP_OK(e.d_part_rows.alloc((size_t)e.parts * (size_t)M));
        HIP_OK(e.d_coef.alloc(5 * (size_t)M));
        HIP_OK(e.d_rec_rows.alloc(4 * (size_t)index_grid((int)M), true));
    }
    h->ewald = std::move(e);                                     // (the old setting's buffers are released here)
    f.energy_launched = false;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_nonbonded_ewald(tgnh_handle h, tgnh_ewald_desc* out, int* num_kvectors) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "tgnh_get_nonbonded_ewald: null out");
    const tgnh_context::Ewald& e = h->ewald;
    std::memset(out, 0, sizeof(*out));
    if (e.on && !e.pme) {                                        // (with PME in force the explicit sum is off: tgnh_get_nonbonded_pme answers)
        out->struct_size = sizeof(tgnh_ewald_desc);
        for (int k = 0; k < 3; k++) out->kmax[k] = e.kmax[k];
        out->alpha = e.alpha;
    }
    if (num_kvectors) *num_kvectors = e.on && !e.pme ? e.vectors : 0;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_ewald_energy(tgnh_handle h, void* stream, double out[4]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    tgnh_status rc = feature_ready(h, "tgnh_get_ewald_energy", &tgnh_context::Bound::posq, true); if (rc) return rc;
    const tgnh_context::Ewald& e = h->ewald;
    if (!e.on) return fail(TGNH_ERR_STATE, "tgnh_get_ewald_energy: Ewald summation is off (tgnh_set_nonbonded_ewald)");
    if (!e.energy_launched || !h->nonbonded.energy_launched)
        return fail(TGNH_ERR_STATE, "tgnh_get_ewald_energy: no tgnh_compute_nonbonded_force with want_energy since Ewald summation was set");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    // the reciprocal rows: the finalise launch's, x misc[1] = (4 (pi K)) / V; with PME the z launch's 1/2 sum of G |F|^2, x K
    const int n_rec = e.pme ? pme_fft_grid(e.grid, 2) : (e.vectors > 0 ? index_grid(e.vectors) : 0);
    HIP_OK(launch_ewald_energy_sum(e.d_rec_rows, n_rec, e.pme ? NB_COULOMB : 0.0, e.d_exc_rows, e.corrected ? index_grid(e.recv.n) : 0,
                                   e.d_misc, e.e_self, e.d_totals, s));
    double got[4];
    rc = fetch_totals(h, e.d_totals, s, got); if (rc) return rc;
    for (int k = 0; k < 4; k++) out[k] = got[k];
    return TGNH_OK;
}
