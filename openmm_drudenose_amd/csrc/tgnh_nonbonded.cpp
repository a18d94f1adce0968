// tgnh_nonbonded.cpp -- the library's NonbondedForce: the particle table and the exceptions (checks, krf and crf formed in fp64, the
// exclusion lists per slot, the evaluated exceptions' shares by receiving slot), tgnh_compute_nonbonded_force (the box's checks,
// the cell grid, the per-cell buffers, the launches) and tgnh_get_nonbonded_energy (tgnh_nonbonded.hip has the kernels;
// include/drude_tgnh.h the contract).  With Ewald summation on (tgnh_set_nonbonded_ewald, tgnh_ewald.cpp) the compute call hands the pair
// launch alpha and adds tgnh_ewald.hip's launches behind the exceptions, and with PME on (tgnh_set_nonbonded_pme, tgnh_pme.cpp) that
// unit's behind those.
#include <climits>

#include "tgnh_host.h"
#include "tgnh_ewald.h"

#pragma clang fp contract(off)      // krf and crf are part of the contract: every operation rounded on its own

static bool nb_sharded(const tgnh_context* c) { return c->xchg.on || c->xchg.allreduce || c->xchg.rccl_comm; }

extern "C" tgnh_status tgnh_set_nonbonded_force(tgnh_handle h, const tgnh_nonbonded_desc* d) {
    CHECK_H(h);
    const char* me = "tgnh_set_nonbonded_force: ";
    if (d && d->struct_size != sizeof(tgnh_nonbonded_desc))
        return fail(TGNH_ERR_ARG, std::string(me) + "struct_size " + std::to_string(d->struct_size) + " is not sizeof(tgnh_nonbonded_desc)");
    if (!d || d->num_particles == 0) {
        if (!h->host_only) HIP_OK(hipSetDevice(h->device));
        h->nonbonded = tgnh_context::Nonbonded();
        h->ewald = tgnh_context::Ewald();                        // (Ewald summation rests on the table: it goes with it)
        return TGNH_OK;
    }
    if (d->method != TGNH_NB_CUTOFF_PERIODIC)
        return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "method " + std::to_string(d->method) + ": only TGNH_NB_CUTOFF_PERIODIC is built");
    const int N = h->d.num_particles, ne = d->num_exceptions;
    if (d->num_particles != N)
        return fail(TGNH_ERR_ARG, std::string(me) + std::to_string(d->num_particles) + " particles for a handle of " + std::to_string(N) + " slots");
    if (ne < 0) return fail(TGNH_ERR_ARG, std::string(me) + "a negative count");
    if (!d->particles || (ne > 0 && (!d->exception_particles || !d->exception_params)))
        return fail(TGNH_ERR_ARG, std::string(me) + "a null array with a positive count");
    if (!std::isfinite(d->cutoff) || d->cutoff <= 0.0) return fail(TGNH_ERR_ARG, std::string(me) + "the cutoff is not finite or not positive");
    if (!std::isfinite(d->reaction_field_dielectric) || d->reaction_field_dielectric < 1.0)
        return fail(TGNH_ERR_ARG, std::string(me) + "the reaction field dielectric is not finite or below 1");
    // (before any row is read: the counts alone decide it)
    if (2LL * ne > INT_MAX) return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "more exceptions than the exclusion lists' 32-bit offsets take");
    if (nb_sharded(h))
        return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "this handle is one shard of several: pairs cross shards, and nothing is exchanged here");
    for (int i = 0; i < N; i++) {
        const double* p = d->particles + 3 * (size_t)i;
        const std::string who = std::string(me) + "particle " + std::to_string(i);
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return fail(TGNH_ERR_ARG, who + ": a parameter is not finite");
        if (p[1] < 0.0) return fail(TGNH_ERR_ARG, who + ": sigma is negative");
        if (p[2] < 0.0) return fail(TGNH_ERR_ARG, who + ": epsilon is negative");
    }
    struct Row { int lo, hi, row; };
    std::vector<Row> rows((size_t)ne);
    for (int r = 0; r < ne; r++) {
        const int32_t* at = d->exception_particles + 2 * (size_t)r;
        const double* p = d->exception_params + 3 * (size_t)r;
        const std::string who = std::string(me) + "exception " + std::to_string(r);
        for (int m = 0; m < 2; m++)
            if (at[m] < 0 || at[m] >= N) return fail(TGNH_ERR_ARG, who + ": index " + std::to_string(at[m]) + " out of range");
        if (at[0] == at[1]) return fail(TGNH_ERR_ARG, who + " names particle " + std::to_string(at[0]) + " twice");
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return fail(TGNH_ERR_ARG, who + ": a parameter is not finite");
        if (p[1] < 0.0) return fail(TGNH_ERR_ARG, who + ": sigma is negative");
        if (p[2] < 0.0) return fail(TGNH_ERR_ARG, who + ": epsilon is negative");
        rows[r] = {std::min(at[0], at[1]), std::max(at[0], at[1]), r};
    }
    std::sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.lo != y.lo ? x.lo < y.lo : (x.hi != y.hi ? x.hi < y.hi : x.row < y.row); });
    int twice = -1, first = -1;
    for (size_t r = 1; r < rows.size(); r++)
        if (rows[r].lo == rows[r - 1].lo && rows[r].hi == rows[r - 1].hi && (twice < 0 || rows[r].row < twice)) { twice = rows[r].row; first = rows[r - 1].row; }
    if (twice >= 0)
        return fail(TGNH_ERR_ARG, std::string(me) + "exception " + std::to_string(twice) + " names the pair of exception " + std::to_string(first) + " again");
    int evaluated = 0;
    for (int r = 0; r < ne; r++) evaluated += d->exception_params[3 * (size_t)r] != 0.0 || d->exception_params[3 * (size_t)r + 2] != 0.0;

    tgnh_context::Nonbonded f;                                   // built aside: a refusal or an upload that fails leaves the tables in force as they were
    f.particles = N; f.exceptions = ne; f.evaluated = evaluated;
    f.cutoff = d->cutoff; f.dielectric = d->reaction_field_dielectric;
    const double rc = d->cutoff, eps = d->reaction_field_dielectric;
    f.krf = ((1.0 / ((rc * rc) * rc)) * (eps - 1.0)) / (2.0 * eps + 1.0);
    f.crf = ((1.0 / rc) * (3.0 * eps)) / (2.0 * eps + 1.0);
    if (h->host_only) { h->nonbonded = std::move(f); h->ewald = tgnh_context::Ewald(); return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    // the exclusion lists: every exception row, evaluated or not, under both of its slots, ascending
    std::vector<int> excl_start((size_t)N + 1, 0), excl(2 * (size_t)ne);
    std::vector<int2> excl_range((size_t)N, make_int2(1, 0));
    for (int r = 0; r < ne; r++) { excl_start[rows[r].lo + 1]++; excl_start[rows[r].hi + 1]++; }
    for (int i = 0; i < N; i++) excl_start[i + 1] += excl_start[i];
    {
        std::vector<int> cursor(excl_start.begin(), excl_start.end() - 1);
        for (const Row& r : rows) { excl[cursor[r.lo]++] = r.hi; excl[cursor[r.hi]++] = r.lo; }
        for (int i = 0; i < N; i++) {
            std::sort(excl.begin() + excl_start[i], excl.begin() + excl_start[i + 1]);
            if (excl_start[i + 1] > excl_start[i]) excl_range[i] = make_int2(excl[excl_start[i]], excl[excl_start[i + 1] - 1]);
        }
    }
    // the evaluated rows in the caller's order, and their shares
    std::vector<int2> exc_atoms; std::vector<double> exc_par;
    std::vector<Share> shares;
    for (int r = 0; r < ne; r++) {
        const double* p = d->exception_params + 3 * (size_t)r;
        if (p[0] == 0.0 && p[2] == 0.0) continue;
        const int32_t* at = d->exception_particles + 2 * (size_t)r;
        const int t = (int)exc_atoms.size();
        exc_atoms.push_back(make_int2(at[0], at[1]));
        exc_par.insert(exc_par.end(), p, p + 3);
        shares.push_back({at[0], t, 0}); shares.push_back({at[1], t, 1});
    }
    HIP_OK(f.d_par.upload(d->particles, 3 * (size_t)N));
    HIP_OK(f.d_excl_start.upload(excl_start));
    HIP_OK(f.d_excl.upload(excl));
    HIP_OK(f.d_excl_range.upload(excl_range));
    if (evaluated) {
        HIP_OK(f.d_exc_atoms.upload(exc_atoms));
        HIP_OK(f.d_exc_par.upload(exc_par));
        HIP_OK(f.recv.upload(invert_shares(std::move(shares))));
        HIP_OK(f.d_exc_rows.alloc(4 * (size_t)index_grid(f.recv.n), true));
    }
    // the per-slot buffers of the cell build now: a call may be recorded into a graph
    HIP_OK(f.d_cell_of.alloc((size_t)N));
    HIP_OK(f.d_placed.alloc((size_t)N));
    HIP_OK(f.d_sorted.alloc(6 * (size_t)N));
    HIP_OK(f.d_sorted_slot.alloc((size_t)N));
    HIP_OK(f.d_sorted_range.alloc((size_t)N));
    HIP_OK(f.d_n_chunks.alloc(1, true));
    HIP_OK(f.d_totals.alloc(4, true));
    f.h_charge.resize((size_t)N); f.h_exc.resize((size_t)ne);
    for (int i = 0; i < N; i++) f.h_charge[i] = d->particles[3 * (size_t)i];
    for (int r = 0; r < ne; r++) f.h_exc[r] = make_int2(d->exception_particles[2 * (size_t)r], d->exception_particles[2 * (size_t)r + 1]);
    h->nonbonded = std::move(f);                                 // (the old tables' buffers are released here)
    h->ewald = tgnh_context::Ewald();
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_num_nonbonded_terms(tgnh_handle h, int out[3]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null counts");
    out[0] = h->nonbonded.particles; out[1] = h->nonbonded.exceptions; out[2] = h->nonbonded.evaluated;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_compute_nonbonded_force(tgnh_handle h, void* force, int want_energy, void* stream) {
    const char* me = "tgnh_compute_nonbonded_force: ";
    tgnh_status rc = feature_ready(h, "tgnh_compute_nonbonded_force", &tgnh_context::Bound::posq, true); if (rc) return rc;
    if (!force) return fail(TGNH_ERR_STATE, std::string(me) + "no force buffer");
    tgnh_context::Nonbonded& f = h->nonbonded;
    if (f.particles == 0) return TGNH_OK;
    if (!h->box.set) return fail(TGNH_ERR_STATE, std::string(me) + "no periodic box: tgnh_set_periodic_box has not been called");
    if (nb_sharded(h)) return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "this handle is one shard of several: pairs cross shards, and nothing is exchanged here");
    if (h->box.b[0] != 0.0 || h->box.c[0] != 0.0 || h->box.c[1] != 0.0)
        return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "a triclinic box (a non-zero off-diagonal component) is not built");
    const double L[3] = {h->box.a[0], h->box.b[1], h->box.c[2]};
    if (f.cutoff > 0.5 * std::min(L[0], std::min(L[1], L[2])))
        return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "the cutoff is above half the shortest box edge");
    NonbondedArgs a{};
    long long ncells = 1;
    for (int k = 0; k < 3; k++) {
        const double cells = std::floor(L[k] / (NB_CELL_MARGIN * f.cutoff));
        a.nc[k] = cells < 1.0 ? 1 : (cells > (double)NB_MAX_CELLS ? (int)NB_MAX_CELLS + 1 : (int)cells);
        a.box[k] = L[k];
        ncells *= a.nc[k];
        if (ncells > NB_MAX_CELLS) return fail(TGNH_ERR_UNSUPPORTED, std::string(me) + "more than 2^24 cells: the box is too large for this cutoff");
    }
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipSetDevice(h->device));
    const int n = f.particles;
    if (ncells > f.cells_allocated) {
        if (stream_capturing(s))
            return fail(TGNH_ERR_STATE, std::string(me) + "this box needs more cells than the buffers hold, and they cannot grow inside a stream capture: "
                                                          "call once outside the capture");
        // (built aside: a failed allocation leaves the buffers as they were)
        tgnh::DeviceBuf<int> count, cell_start; tgnh::DeviceBuf<int2> chunks; tgnh::DeviceBuf<double> pair_rows;
        HIP_OK(count.alloc(2 * (size_t)ncells));
        HIP_OK(cell_start.alloc((size_t)ncells + 1));
        HIP_OK(chunks.alloc((size_t)nb_chunk_cap(n, (int)ncells)));
        HIP_OK(pair_rows.alloc(4 * (size_t)nb_pair_grid(n, (int)ncells), true));
        f.d_count = std::move(count); f.d_cell_start = std::move(cell_start); f.d_chunks = std::move(chunks); f.d_pair_rows = std::move(pair_rows);
        f.cells_allocated = (int)ncells;
        f.energy_launched = false;                               // (the pair rows of the last want_energy call went with the old buffer)
    }
    a.n = n; a.par = f.d_par; a.excl_start = f.d_excl_start; a.excl = f.d_excl; a.excl_range = f.d_excl_range;
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr;
    a.ncells = (int)ncells;
    a.cutoff2 = f.cutoff * f.cutoff; a.krf = f.krf; a.crf = f.crf;
    a.cell_of = f.d_cell_of; a.count = f.d_count; a.cell_start = f.d_cell_start; a.chunks = f.d_chunks; a.n_chunks = f.d_n_chunks;
    a.chunk_cap = nb_chunk_cap(n, a.ncells);
    a.placed = f.d_placed; a.sorted = f.d_sorted; a.sorted_slot = f.d_sorted_slot; a.sorted_range = f.d_sorted_range;
    a.force = static_cast<long long*>(force); a.padded = h->d.padded_num_particles;
    a.rows = want_energy ? f.d_pair_rows.get() : nullptr;
    tgnh_context::Ewald& ew = h->ewald;
    if (ew.on) { a.alpha = ew.alpha; a.tsp = ew.tsp; a.bg_num = ew.bg_num; a.ew_misc = ew.d_misc; }
    f.last_stream = s;
    HIP_OK(hipMemsetAsync(f.d_count, 0, 2 * (size_t)ncells * sizeof(int), s));
    for (int stage = 0; stage < 4; stage++) {
        Timed t(h, s, KID_OTHER);
        HIP_OK(launch_nonbonded_cells(h->d.precision, a, s, stage));
    }
    {
        Timed t(h, s, KID_OTHER);
        HIP_OK(launch_nonbonded_pairs(h->d.precision, a, s));
    }
    if (f.evaluated) {
        NbExceptionArgs x{};
        x.atoms = f.d_exc_atoms; x.par = f.d_exc_par;
        x.recv = f.recv.view();
        x.posq = h->bound.posq; x.posq_corr = h->bound.posq_corr;
        x.force = a.force; x.padded = a.padded;
        x.rows = want_energy ? f.d_exc_rows.get() : nullptr;
        Timed t(h, s, KID_OTHER);
        HIP_OK(launch_nonbonded_exceptions(h->d.precision, x, s));
    }
    if (ew.on && ew.corrected) {
        EwaldExclusionArgs x{};
        x.atoms = ew.d_exc_atoms; x.par = f.d_par;
        x.recv = ew.recv.view();
        x.posq = h->bound.posq; x.posq_corr = h->bound.posq_corr;
        x.alpha = ew.alpha; x.tsp = ew.tsp;
        x.force = a.force; x.padded = a.padded;
        x.rows = want_energy ? ew.d_exc_rows.get() : nullptr;
        Timed t(h, s, KID_OTHER);
        HIP_OK(launch_ewald_exclusions(h->d.precision, x, s));
    }
    if (ew.on && ew.vectors > 0) {
        EwaldArgs r{};
        r.n = n; r.m = ew.vectors; r.parts = ew.parts;
        r.kvec = ew.d_kvec; r.par = f.d_par;
        r.posq = h->bound.posq; r.posq_corr = h->bound.posq_corr;
        for (int k = 0; k < 3; k++) r.box[k] = L[k];
        r.a4 = ew.a4;
        r.part_rows = ew.d_part_rows; r.coef = ew.d_coef;
        r.rows = want_energy ? ew.d_rec_rows.get() : nullptr;
        r.force = a.force; r.padded = a.padded;
        for (int stage = 0; stage < 3; stage++) {
            Timed t(h, s, KID_OTHER);
            HIP_OK(launch_ewald_reciprocal(h->d.precision, r, s, stage));
        }
    }
    if (ew.on && ew.pme) { rc = pme_launches(h, L, force, want_energy, s); if (rc) return rc; }
    // (a launch recorded into a stream capture has not run: it fills the rows when the graph is replayed, and does not count here)
    if (want_energy && !stream_capturing(s)) { f.energy_launched = true; f.energy_rows = nb_pair_grid(n, a.ncells); ew.energy_launched = ew.on; }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_nonbonded_energy(tgnh_handle h, void* stream, double out[4]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    tgnh_status rc = feature_ready(h, "tgnh_get_nonbonded_energy", &tgnh_context::Bound::posq, true); if (rc) return rc;
    const tgnh_context::Nonbonded& f = h->nonbonded;
    if (!f.energy_launched) return fail(TGNH_ERR_STATE, "tgnh_get_nonbonded_energy: no tgnh_compute_nonbonded_force with want_energy since the tables were set");
    HIP_OK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(launch_nonbonded_energy_sum(f.d_pair_rows, f.energy_rows, f.d_exc_rows, f.evaluated ? index_grid(f.recv.n) : 0, f.d_totals, s));
    double got[4];
    rc = fetch_totals(h, f.d_totals, s, got); if (rc) return rc;
    for (int k = 0; k < 4; k++) out[k] = got[k];
    return TGNH_OK;
}
