// tgnh_bonded.cpp -- the library's bonded forces: the tables of harmonic bonds, harmonic angles and periodic torsions (checks, the
// phases' cosine and sine formed in fp64, the three tables' shares by receiving slot), tgnh_compute_bonded_forces and
// tgnh_get_bonded_energy (tgnh_bonded.hip has the kernels; include/drude_tgnh.h the contract)
#include <climits>

#include "tgnh_host.h"
#include "tgnh_bonded.h"

static const double BONDED_PI = 3.14159265358979323846;

// what is wrong with one table's rows (TGNH_ERR_ARG, TGNH_ERR_UNSUPPORTED), before any device work.  kind: "bond", "angle", "torsion";
// atoms [n][width]; params [n][2]: (length | angle | phase, k); periodicity: the torsions', else nullptr
static tgnh_status bonded_check(const tgnh_context* c, const char* kind, int n, int width, const int32_t* atoms, const double* params,
                                const int32_t* periodicity) {
    const int N = c->d.num_particles;
    const char* first = width == 2 ? "length" : (width == 3 ? "angle" : "phase");
    for (int r = 0; r < n; r++) {
        const std::string who = std::string("tgnh_set_bonded_forces: ") + kind + " " + std::to_string(r);
        const int32_t* at = atoms + (size_t)width * r;
        for (int m = 0; m < width; m++)
            if (at[m] < 0 || at[m] >= N) return fail(TGNH_ERR_ARG, who + ": index " + std::to_string(at[m]) + " out of range");
        for (int m = 0; m < width; m++)
            for (int q = m + 1; q < width; q++)
                if (at[m] == at[q]) return fail(TGNH_ERR_ARG, who + " names particle " + std::to_string(at[m]) + " twice");
        const double x = params[2 * (size_t)r], k = params[2 * (size_t)r + 1];
        if (!std::isfinite(x)) return fail(TGNH_ERR_ARG, who + ": the " + first + " is not finite");
        if (!std::isfinite(k)) return fail(TGNH_ERR_ARG, who + ": k is not finite");
        if (width == 2 && x < 0.0) return fail(TGNH_ERR_ARG, who + ": the length is negative");
        if (width == 3 && (x < 0.0 || x > BONDED_PI)) return fail(TGNH_ERR_ARG, who + ": the angle is outside [0, pi]");
        if (periodicity) {
            if (periodicity[r] < 1) return fail(TGNH_ERR_ARG, who + ": periodicity " + std::to_string(periodicity[r]) + " is below 1");
            if (periodicity[r] > BONDED_MAX_PERIODICITY)
                return fail(TGNH_ERR_UNSUPPORTED, who + ": periodicity " + std::to_string(periodicity[r]) + " is above " + std::to_string(BONDED_MAX_PERIODICITY));
        }
    }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_bonded_forces(tgnh_handle h, int num_bonds, const int32_t* bond_particles, const double* bond_params,
                                              int num_angles, const int32_t* angle_particles, const double* angle_params,
                                              int num_torsions, const int32_t* torsion_particles, const int32_t* torsion_periodicity,
                                              const double* torsion_params) {
    CHECK_H(h);
    if (num_bonds < 0 || num_angles < 0 || num_torsions < 0) return fail(TGNH_ERR_ARG, "tgnh_set_bonded_forces: a negative count");
    if ((num_bonds > 0 && (!bond_particles || !bond_params)) || (num_angles > 0 && (!angle_particles || !angle_params)) ||
        (num_torsions > 0 && (!torsion_particles || !torsion_periodicity || !torsion_params)))
        return fail(TGNH_ERR_ARG, "tgnh_set_bonded_forces: a null array with a positive count");
    // (before any row is read: the counts alone decide it)
    if (2LL * num_bonds + 3LL * num_angles + 4LL * num_torsions > INT_MAX)
        return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_bonded_forces: more entries than the inverted table's 32-bit offsets take");
    tgnh_status rc = bonded_check(h, "bond", num_bonds, 2, bond_particles, bond_params, nullptr); if (rc) return rc;
    rc = bonded_check(h, "angle", num_angles, 3, angle_particles, angle_params, nullptr); if (rc) return rc;
    rc = bonded_check(h, "torsion", num_torsions, 4, torsion_particles, torsion_params, torsion_periodicity); if (rc) return rc;
    if (h->host_only) { h->bonded.bonds = num_bonds; h->bonded.angles = num_angles; h->bonded.torsions = num_torsions; return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    if (num_bonds + num_angles + num_torsions == 0) { h->bonded = tgnh_context::BondedForces(); return TGNH_OK; }
    const size_t nb = (size_t)num_bonds, na = (size_t)num_angles, nt = (size_t)num_torsions;
    std::vector<int2> b_atoms(nb);
    std::vector<double2> b_par(nb), a_par(na);
    std::vector<int4> a_atoms(na), t_atoms(nt);
    std::vector<int> t_n(nt);
    std::vector<double> t_par(3 * nt);
    std::vector<Share> shares;                                   // pushed in term order
    shares.reserve(2 * nb + 3 * na + 4 * nt);
    for (size_t r = 0; r < nb; r++) {
        const int32_t* at = bond_particles + 2 * r;
        b_atoms[r] = make_int2(at[0], at[1]);
        b_par[r] = make_double2(bond_params[2 * r], bond_params[2 * r + 1]);
        for (int m = 0; m < 2; m++) shares.push_back({at[m], (int)r, (unsigned char)m});
    }
    for (size_t r = 0; r < na; r++) {
        const int32_t* at = angle_particles + 3 * r;
        a_atoms[r] = make_int4(at[0], at[1], at[2], 0);
        a_par[r] = make_double2(angle_params[2 * r], angle_params[2 * r + 1]);
        for (int m = 0; m < 3; m++) shares.push_back({at[m], (int)(nb + r), (unsigned char)m});
    }
    for (size_t r = 0; r < nt; r++) {
        const int32_t* at = torsion_particles + 4 * r;
        t_atoms[r] = make_int4(at[0], at[1], at[2], at[3]);
        t_n[r] = torsion_periodicity[r];
        t_par[r] = std::cos(torsion_params[2 * r]); t_par[nt + r] = std::sin(torsion_params[2 * r]); t_par[2 * nt + r] = torsion_params[2 * r + 1];
        for (int m = 0; m < 4; m++) shares.push_back({at[m], (int)(nb + na + r), (unsigned char)m});
    }
    tgnh_context::BondedForces f;                                // built aside: an upload that fails leaves the tables in force as they were
    HIP_OK(f.d_bond_atoms.upload(b_atoms));
    HIP_OK(f.d_bond_par.upload(b_par));
    HIP_OK(f.d_angle_atoms.upload(a_atoms));
    HIP_OK(f.d_angle_par.upload(a_par));
    HIP_OK(f.d_torsion_atoms.upload(t_atoms));
    HIP_OK(f.d_torsion_n.upload(t_n));
    HIP_OK(f.d_torsion_par.upload(t_par));
    HIP_OK(f.recv.upload(invert_shares(std::move(shares))));
    HIP_OK(f.d_energy.alloc(4 * ((size_t)bf_grid(f.recv.n) + 1), true));     // the energy rows now: the launch may be recorded into a graph
    f.bonds = num_bonds; f.angles = num_angles; f.torsions = num_torsions;
    h->bonded = std::move(f);                                    // (the old tables' buffers are released here)
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_num_bonded_terms(tgnh_handle h, int out[3]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null counts");
    out[0] = h->bonded.bonds; out[1] = h->bonded.angles; out[2] = h->bonded.torsions;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_compute_bonded_forces(tgnh_handle h, void* force, int want_energy, void* stream) {
    tgnh_status rc = feature_ready(h, "tgnh_compute_bonded_forces", &tgnh_context::Bound::posq, true); if (rc) return rc;
    if (!force) return fail(TGNH_ERR_STATE, "tgnh_compute_bonded_forces: no force buffer");
    const tgnh_context::BondedForces& f = h->bonded;
    if (f.empty()) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    BondedArgs a{};
    a.bond_atoms = f.d_bond_atoms; a.bond_par = f.d_bond_par; a.angle_atoms = f.d_angle_atoms; a.angle_par = f.d_angle_par;
    a.torsion_atoms = f.d_torsion_atoms; a.torsion_n = f.d_torsion_n; a.torsion_par = f.d_torsion_par;
    a.n_bonds = f.bonds; a.n_angles = f.angles; a.n_torsions = f.torsions;
    a.recv = f.recv.view();
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr;
    a.force = static_cast<long long*>(force); a.padded = h->d.padded_num_particles;
    a.rows = want_energy ? f.d_energy.get() : nullptr;
    Timed t(h, (hipStream_t)stream, KID_OTHER);
    HIP_OK(launch_bonded_forces(h->d.precision, a, (hipStream_t)stream));
    // (a launch recorded into a stream capture has not run: it fills the rows when the graph is replayed, and does not count here)
    if (want_energy && !stream_capturing((hipStream_t)stream)) h->bonded.energy_launched = true;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_bonded_energy(tgnh_handle h, void* stream, double out[3]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    tgnh_status rc = feature_ready(h, "tgnh_get_bonded_energy", &tgnh_context::Bound::posq, true); if (rc) return rc;
    const tgnh_context::BondedForces& f = h->bonded;
    if (!f.energy_launched) return fail(TGNH_ERR_STATE, "tgnh_get_bonded_energy: no tgnh_compute_bonded_forces with want_energy since the tables were set");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int grid = bf_grid(f.recv.n);
    double* totals = f.d_energy.get() + 4 * (size_t)grid;
    HIP_OK(launch_bonded_energy_sum(f.d_energy, grid, totals, s));
    double got[4];
    rc = fetch_totals(h, totals, s, got); if (rc) return rc;
    out[0] = got[0]; out[1] = got[1]; out[2] = got[2];
    return TGNH_OK;
}
