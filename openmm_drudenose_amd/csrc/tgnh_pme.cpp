// tgnh_pme.cpp -- smooth particle-mesh Ewald on top of the library's NonbondedForce: tgnh_set_nonbonded_pme (the checks, the per-axis
// tables of twiddle factors and B-spline moduli, the three grids; what it shares with tgnh_set_nonbonded_ewald is tgnh_ewald.cpp's),
// tgnh_get_nonbonded_pme, tgnh_get_pme_grids, and the launches tgnh_compute_nonbonded_force (tgnh_nonbonded.cpp) makes with PME on.
// tgnh_pme.hip has the kernels; include/drude_tgnh.h the contract.
#include "tgnh_host.h"
#include "tgnh_pme.h"

#pragma clang fp contract(off)      // the moduli are part of the contract: every operation rounded on its own

namespace {
// w^k = (cos(2 pi k / N), -sin(2 pi k / N)), k < N: the angle reduced to the first octant in integers, cosl and sinl there, rounded
// once -- exact at every multiple of a quarter turn, and correctly rounded or an ulp off elsewhere
std::vector<double2> pme_twiddles(int N) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    std::vector<double2> w((size_t)N);
    for (int k = 0; k < N; k++) {
        // the angle is 2 pi k / N = (pi / 4) (8 k / N): octant o, and within it r / N of an eighth turn
        const int o = (8 * k) / N, r = 8 * k - o * N;
        const int odd = o & 1;
        // an odd octant is measured back from its end
        const long double t = two_pi * (long double)(odd ? N - r : r) / (8.0L * (long double)N);
        const long double c = cosl(t), s = sinl(t);
        long double x, y;                                        // cos, sin of the whole angle
        switch (o) {
            case 0: x = c; y = s; break;
            case 1: x = s; y = c; break;
            case 2: x = -s; y = c; break;
            case 3: x = -c; y = s; break;
            case 4: x = -c; y = -s; break;
            case 5: x = -s; y = -c; break;
            case 6: x = s; y = -c; break;
            default: x = c; y = -s; break;
        }
        w[(size_t)k] = make_double2((double)x, (double)(-y));
    }
    return w;
}

// |b(m)|^2 of B-spline order 5 from the table's entries, then OpenMM's rule for the zeros
std::vector<double> pme_moduli(const std::vector<double2>& w) {
    const int N = (int)w.size();
    const double M[4] = {1.0 / 24.0, 11.0 / 24.0, 11.0 / 24.0, 1.0 / 24.0};
    std::vector<double> b((size_t)N);
    for (int m = 0; m < N; m++) {
        double sc = 0.0, ss = 0.0;
        for (int j = 0; j < 4; j++) {
            const double2 t = w[(size_t)((m * j) % N)];
            sc = sc + M[j] * t.x;
            ss = ss + M[j] * (-t.y);
        }
        b[(size_t)m] = sc * sc + ss * ss;
    }
    for (int m = 0; m < N; m++)
        if (b[(size_t)m] < 1e-7) b[(size_t)m] = (b[(size_t)((m - 1 + N) % N)] + b[(size_t)((m + 1) % N)]) * 0.5;
    return b;
}
}  // namespace

extern "C" tgnh_status tgnh_set_nonbonded_pme(tgnh_handle h, const tgnh_pme_desc* d) {
    CHECK_H(h);
    const char* me = "tgnh_set_nonbonded_pme: ";
    tgnh_context::Nonbonded& f = h->nonbonded;
    bool done;
    tgnh_status rc = ewald_set_begin(h, me, d == nullptr, &done);
    if (rc || done) return rc;
    if (d->struct_size != sizeof(tgnh_pme_desc))
        return fail(TGNH_ERR_ARG, std::string(me) + "struct_size " + std::to_string(d->struct_size) + " is not sizeof(tgnh_pme_desc)");
    if (!std::isfinite(d->alpha) || d->alpha <= 0.0) return fail(TGNH_ERR_ARG, std::string(me) + "alpha is not finite or not positive");
    PmeFftPlan plan[3];
    long long points = 1;
    for (int k = 0; k < 3; k++) {
        const std::string name = "grid[" + std::to_string(k) + "] = " + std::to_string(d->grid[k]);
        if (d->grid[k] < PME_MIN_GRID || d->grid[k] > PME_MAX_GRID) return fail(TGNH_ERR_ARG, std::string(me) + name + " is not in [6, 256]");
        if (!pme_fft_plan(d->grid[k], &plan[k])) return fail(TGNH_ERR_ARG, std::string(me) + name + " has a prime factor other than 2, 3 and 5");
        points *= d->grid[k];
    }
    if (points > PME_MAX_POINTS) return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + std::to_string(points) + " grid points: more than 2^24");

    tgnh_context::Ewald e;                                       // built aside: a refusal or an upload that fails leaves what was in force
    ewald_set_constants(e, d->alpha);
    e.pme = true;
    for (int k = 0; k < 3; k++) e.grid[k] = d->grid[k];
    e.pi2 = EW_PI * EW_PI;
    e.alpha2 = d->alpha * d->alpha;
    if (h->host_only) { h->ewald = std::move(e); f.energy_launched = false; return TGNH_OK; }
    rc = ewald_set_shared(h, e); if (rc) return rc;
    for (int k = 0; k < 3; k++) {
        const std::vector<double2> w = pme_twiddles(e.grid[k]);
        HIP_OK(e.d_twiddle[k].upload(w));
        HIP_OK(e.d_modulus[k].upload(pme_moduli(w)));
    }
    HIP_OK(e.d_charge.alloc((size_t)points, true));
    HIP_OK(e.d_work.alloc((size_t)points, true));
    HIP_OK(e.d_potential.alloc((size_t)points, true));
    HIP_OK(e.d_rec_rows.alloc(4 * (size_t)pme_fft_grid(e.grid, 2), true));
    h->ewald = std::move(e);                                     // (the old setting's buffers are released here)
    f.energy_launched = false;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_nonbonded_pme(tgnh_handle h, tgnh_pme_desc* out) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "tgnh_get_nonbonded_pme: null out");
    const tgnh_context::Ewald& e = h->ewald;
    std::memset(out, 0, sizeof(*out));
    if (e.on && e.pme) {
        out->struct_size = sizeof(tgnh_pme_desc);
        for (int k = 0; k < 3; k++) out->grid[k] = e.grid[k];
        out->alpha = e.alpha;
    }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_pme_grids(tgnh_handle h, void* stream, long long* charge, double* potential) {
    tgnh_status rc = feature_ready(h, "tgnh_get_pme_grids", &tgnh_context::Bound::posq, true); if (rc) return rc;
    const tgnh_context::Ewald& e = h->ewald;
    if (!e.on || !e.pme) return fail(TGNH_ERR_STATE, "tgnh_get_pme_grids: particle-mesh Ewald is off (tgnh_set_nonbonded_pme)");
    if (!e.grids_filled) return fail(TGNH_ERR_STATE, "tgnh_get_pme_grids: no tgnh_compute_nonbonded_force since particle-mesh Ewald was set");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t points = ((size_t)e.grid[0] * (size_t)e.grid[1]) * (size_t)e.grid[2];
    if (charge) HIP_OK(hipMemcpyAsync(charge, e.d_charge, points * sizeof(long long), hipMemcpyDeviceToHost, s));
    if (potential) HIP_OK(hipMemcpyAsync(potential, e.d_potential, points * sizeof(double), hipMemcpyDeviceToHost, s));
    return finish_query(h, s);
}

// tgnh_compute_nonbonded_force's launches with PME on, behind the exclusion correction: the memset, spread, five transform launches,
// gather.  Everything was allocated at set time: nothing here grows, and the call stays capturable.
tgnh_status pme_launches(tgnh_handle h, const double L[3], void* force, int want_energy, hipStream_t s) {
    tgnh_context::Ewald& e = h->ewald;
    const tgnh_context::Nonbonded& f = h->nonbonded;
    PmeArgs a{};
    a.n = f.particles;
    size_t points = 1;
    for (int k = 0; k < 3; k++) {
        a.grid[k] = e.grid[k]; a.box[k] = L[k];
        if (!pme_fft_plan(e.grid[k], &a.plan[k])) return fail(TGNH_ERR_STATE, "tgnh_compute_nonbonded_force: internal: a PME grid without a transform plan");
        a.twiddle[k] = e.d_twiddle[k]; a.modulus[k] = e.d_modulus[k];
        points *= (size_t)e.grid[k];
    }
    a.par = f.d_par;
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr;
    a.pi2 = e.pi2; a.alpha2 = e.alpha2;
    a.charge = e.d_charge; a.work = e.d_work; a.potential = e.d_potential;
    a.rows = want_energy ? e.d_rec_rows.get() : nullptr;
    a.force = static_cast<long long*>(force); a.padded = h->d.padded_num_particles;
    HIP_OK(hipMemsetAsync(e.d_charge, 0, points * sizeof(long long), s));
    for (int stage = 0; stage < 7; stage++) {
        Timed t(h, s, KID_OTHER);
        HIP_OK(launch_pme(h->d.precision, a, s, stage));
    }
    if (!stream_capturing(s)) e.grids_filled = true;
    return TGNH_OK;
}
