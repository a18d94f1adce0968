// tgnh_queries.cpp -- what a caller may ask a handle: kinetic energies, thermostat state, topology read-back, timing and algorithmic bytes
#include "tgnh_host.h"

static tgnh_status read_state(tgnh_handle h, int off, int n, hipStream_t s, double* out) {
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    if (h->host_only) { std::copy(h->thermo.h_state.begin() + off, h->thermo.h_state.begin() + off + n, out); return TGNH_OK; }
    { tgnh_status rc = entry(h, false); if (rc) return rc; }
    { tgnh_status rc = materialize_chain(h, s); if (rc) return rc; }
    HIP_OK(hipMemcpyAsync(out, h->thermo.d_state + off, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    return finish_query(h, s);
}

extern "C" tgnh_status tgnh_get_kinetic_energy(tgnh_handle h, int ke_sum_valid, void* stream, double* out) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    hipStream_t s = (hipStream_t)stream;
    if (h->d.mode == TGNH_MODE_TGNH && ke_sum_valid)                               // Cu :654-658
        return read_state(h, h->thermo.L.off_kesum, 1, s, out);
    tgnh_status rc = entry(h, true); if (rc) return rc;
    rc = flush_impl(h, s); if (rc) return rc;
    const double ts = h->d.mode == TGNH_MODE_DUALNH ? 0.5 * h->d.step_size : 0.0; // Ref :587 ; Cu :656
    HIP_OK(launch_plain_ke(h->d.precision, h->bound.velm, reinterpret_cast<const long long*>(h->bound.force), h->d.num_particles,
                           h->d.padded_num_particles, ts, h->thermo.d_scalar, s));
    HIP_OK(hipMemcpyAsync(out, h->thermo.d_scalar, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_num_thermostats(tgnh_handle h, int* count) {
    CHECK_H(h);
    if (count) *count = h->thermo.L.NT;
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_get_last_kinetic_energies(tgnh_handle h, void* stream, double* ke) {
    CHECK_H(h);
    return read_state(h, h->thermo.L.off_ke, h->thermo.L.NT, (hipStream_t)stream, ke);
}
extern "C" tgnh_status tgnh_get_last_scale_factors(tgnh_handle h, void* stream, double* scale) {
    CHECK_H(h);
    return read_state(h, h->thermo.L.off_scale_a, h->thermo.L.NT, (hipStream_t)stream, scale);
}
extern "C" tgnh_status tgnh_get_status_flags(tgnh_handle h, void* stream, uint32_t* flags) {
    CHECK_H(h);
    if (!flags) return fail(TGNH_ERR_ARG, "null flags");
    if (h->host_only) { *flags = 0; return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    const tgnh_status rc = finish_query(h, (hipStream_t)stream);
    if (rc != TGNH_ERR_HIP) *flags = *h->status.h_seen;      // handed back also beside a failure the device reported
    return rc;
}
extern "C" tgnh_status tgnh_get_time(tgnh_handle h, double* time, int64_t* step_count) {
    CHECK_H(h);
    if (time) *time = h->run.time;
    if (step_count) *step_count = h->run.step_count;
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_get_dof(tgnh_handle h, double* dof, double* nkt) {
    CHECK_H(h);
    if (dof) std::copy(h->thermo.dof.begin(), h->thermo.dof.end(), dof);
    if (nkt) std::copy(h->thermo.nkbt.begin(), h->thermo.nkbt.end(), nkt);
    return TGNH_OK;
}

static bool chain_section(tgnh_handle h, int which, int* off, int* len) {
    switch (which) {
        case 0: *off = h->thermo.L.off_eta; *len = h->thermo.L.len_eta; return true;
        case 1: *off = h->thermo.L.off_etaDot; *len = h->thermo.L.len_etaDot; return true;
        case 2: *off = h->thermo.L.off_etaDotDot; *len = h->thermo.L.len_etaDotDot; return true;
        case 3: *off = h->thermo.L.off_etaMass; *len = h->thermo.L.len_etaMass; return true;
        default: return false;
    }
}
extern "C" tgnh_status tgnh_get_thermostat_len(tgnh_handle h, int which, int* len) {
    CHECK_H(h);
    int off;
    if (!len) return fail(TGNH_ERR_ARG, "null out");
    if (!chain_section(h, which, &off, len)) return fail(TGNH_ERR_ARG, "bad thermostat array id");
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_get_thermostat_state(tgnh_handle h, int which, void* stream, double* out) {
    CHECK_H(h);
    int off, len;
    if (!chain_section(h, which, &off, &len)) return fail(TGNH_ERR_ARG, "bad thermostat array id");
    return read_state(h, off, len, (hipStream_t)stream, out);
}
extern "C" tgnh_status tgnh_set_thermostat_state(tgnh_handle h, int which, void* stream, const double* in) {
    CHECK_H(h);
    int off, len;
    if (!chain_section(h, which, &off, &len)) return fail(TGNH_ERR_ARG, "bad thermostat array id");
    if (!in) return fail(TGNH_ERR_ARG, "null in");
    tgnh_status rc = deferred_guard(h, "tgnh_set_thermostat_state"); if (rc) return rc;
    h->owed.ke_carry = false;
    if (h->host_only) { std::copy(in, in + len, h->thermo.h_state.begin() + off); return TGNH_OK; }
    HIP_OK(hipSetDevice(h->device));
    rc = materialize_chain(h, (hipStream_t)stream); if (rc) return rc;
    // both copies: the in-kernel chain rewrites only the fields it advances in the staging block, and the next commit
    // copies that block over d_state whole -- a field set here alone (etaMass, an unused etaDot slot) would revert
    HIP_OK(hipMemcpyAsync(h->thermo.d_state + off, in, sizeof(double) * len, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_OK(hipMemcpyAsync(h->thermo.d_stage + off, in, sizeof(double) * len, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    return TGNH_OK;
}

static const std::vector<int>* topo_vec(tgnh_handle h, int which) {
    switch (which) {
        case 0: return &h->topo.normal;
        case 1: return &h->topo.pair_drude;
        case 2: return &h->topo.pair_parent;
        case 3: return &h->topo.group;
        case 4: return &h->topo.resid;
        case 5: return &h->topo.res_count;
        case 6: return &h->topo.res_first;
        case 7: return &h->topo.tile_start;
        default: return nullptr;
    }
}
extern "C" tgnh_status tgnh_get_topology_len(tgnh_handle h, int which, int* len) {
    CHECK_H(h);
    if (!len) return fail(TGNH_ERR_ARG, "null out");
    if (which == 8) { *len = (int)h->topo.meta.size(); return TGNH_OK; }
    if (which == 9) { *len = 2 * (int)h->topo.wave_tile.size(); return TGNH_OK; }      // wave tiles: (first slot, largest molecule) pairs, one more than tiles; 0 = none
    if (which == 10) { *len = (int)h->topo.wmeta.size(); return TGNH_OK; }
    if (which == 11) { *len = (int)h->topo.tile_pat.size(); return TGNH_OK; }        // per 512-slot tile: period | molecules per period << 8 | pattern << 16 (0: per-slot words)
    if (which == 12) { *len = (int)h->topo.wtile_pat.size(); return TGNH_OK; }       // per wave tile: period | pattern << 8
    if (which == 13) { *len = (int)h->topo.pattern.size(); return TGNH_OK; }         // the patterns, 64 words each
    if (which == 14) { *len = (int)h->topo.wpattern.size(); return TGNH_OK; }
    if (which == 15) { *len = 2 * (int)h->topo.wpat_mass.size(); return TGNH_OK; }  // the wave patterns' descriptor masses, 64 doubles each, as pairs of words
    if (which == 16) { *len = 1; return TGNH_OK; }                                   // wpat_all_uniform: every wave tile patterned, every mass its pattern entry's
    // the velocity planes' layout: the stride of a plane in words, the number of tile bases, the bases, the lane offsets (64 per pattern)
    if (which == 17) { *len = 2 + (int)h->topo.wtile_base.size() + (int)h->topo.wpat_off.size(); return TGNH_OK; }
    const std::vector<int>* v = topo_vec(h, which);
    if (!v) return fail(TGNH_ERR_ARG, "bad topology array id");
    *len = (int)v->size();
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_get_topology(tgnh_handle h, int which, int32_t* out) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    auto put = [&](const void* src, size_t bytes) { if (bytes) std::memcpy(out, src, bytes); return TGNH_OK; };     // (an empty array has no data())
    if (which == 8) return put(h->topo.meta.data(), sizeof(uint32_t) * h->topo.meta.size());
    if (which == 9) return put(h->topo.wave_tile.data(), sizeof(int2) * h->topo.wave_tile.size());
    if (which == 10) return put(h->topo.wmeta.data(), sizeof(uint32_t) * h->topo.wmeta.size());
    if (which == 11) return put(h->topo.tile_pat.data(), sizeof(uint32_t) * h->topo.tile_pat.size());
    if (which == 12) return put(h->topo.wtile_pat.data(), sizeof(uint32_t) * h->topo.wtile_pat.size());
    if (which == 13) return put(h->topo.pattern.data(), sizeof(uint32_t) * h->topo.pattern.size());
    if (which == 14) return put(h->topo.wpattern.data(), sizeof(uint32_t) * h->topo.wpattern.size());
    if (which == 15) return put(h->topo.wpat_mass.data(), sizeof(double) * h->topo.wpat_mass.size());
    if (which == 16) { *out = h->topo.wpat_all_uniform ? 1 : 0; return TGNH_OK; }
    if (which == 17) {
        const std::vector<uint32_t>&base = h->topo.wtile_base, &off = h->topo.wpat_off;
        out[0] = base.empty() ? 0 : (int32_t)base.back(); out[1] = (int32_t)base.size();
        if (!base.empty()) std::memcpy(out + 2, base.data(), sizeof(uint32_t) * base.size());
        if (!off.empty()) std::memcpy(out + 2 + base.size(), off.data(), sizeof(uint32_t) * off.size());
        return TGNH_OK;
    }
    const std::vector<int>* v = topo_vec(h, which);
    if (!v) return fail(TGNH_ERR_ARG, "bad topology array id");
    std::copy(v->begin(), v->end(), out);
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_compute_kinetic_energies(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    return ke_query_launches(h, (hipStream_t)stream);
}

// ... and what it enqueues (tgnh_rescale_to_temperature begins with the same launches): the kinetic-energy pass of the velocities as
// they are, its row sum, the all-reduce where one is set; the sums lie in ke_red and in the block's KE entries afterwards
tgnh_status ke_query_launches(tgnh_handle h, hipStream_t s) {
    tgnh_status rc = settle_kick(h, s); if (rc) return rc;
    rc = materialize_chain(h, s); if (rc) return rc;      // ke_red is about to be overwritten
    const int dir = h->run.sweep_reverse;                      // a query leaves the sweep direction as it found it: the step's next
    rc = run_tile(h, OP_KE, KID_KE, s);                    // KE launch then sums in the same order, to the same bits
    h->run.sweep_reverse = dir;
    if (rc) return rc;
    if (h->gather.chain) {
        rc = run_chain_gather(h, s, true); if (rc) return rc;
    } else {
        ChainArgs a = chain_args(h);
        a.do_sum = 1; a.do_chain = 0;
        if (h->xchg.on) { a.x_send = 1; a.x_wait = 1; }
        if (!h->owed.tail_summed) HIP_OK(launch_chain(a, s));       // (summed by the KE launch itself where the step's own KE launch is: the same bits)
        h->owed.tail_summed = false;
        if (!h->xchg.on) { rc = allreduce_hook(h, s); if (rc) return rc; }
    }
    HIP_OK(hipMemcpyAsync(h->thermo.d_state + h->thermo.L.off_ke, h->thermo.d_state + h->thermo.L.off_ke_red, sizeof(double) * h->thermo.L.NT,
                          hipMemcpyDeviceToDevice, s));
    return TGNH_OK;
}

// The Drude pairs as the bound positions have them (include/drude_tgnh.h has the contract; tgnh_drude_stats.hip the kernels).
// A query: it reads posq (+ posq_corr) and nothing of what a step leaves owed -- only velm ever lags --, so there is nothing to
// flush and nothing of the handle changes but the scratch it allocates at its first call.
extern "C" tgnh_status tgnh_get_drude_statistics(tgnh_handle h, double threshold, double hist_max, void* stream, tgnh_drude_stats* out) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    if (out->struct_size != sizeof(tgnh_drude_stats)) return fail(TGNH_ERR_ARG, "tgnh_drude_stats size mismatch (ABI)");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return fail(TGNH_ERR_ARG, "tgnh_get_drude_statistics: threshold is negative or not finite");
    if (!(hist_max >= 0.0) || !std::isfinite(hist_max)) return fail(TGNH_ERR_ARG, "tgnh_get_drude_statistics: hist_max is negative or not finite");
    tgnh_status rc = entry(h, true); if (rc) return rc;          // (buffers bound, not a host-only handle, no failure seen before)
    hipStream_t s = (hipStream_t)stream;
    DrudeStatsRow& r = h->dstats.h_row;                          // (the handle's: a copy still in flight when an error returns lands in live memory)
    r = DrudeStatsRow{};
    r.worst = 0x7fffffff;
    if (h->d.num_pairs > 0) {
        const int grid = index_grid(h->d.num_particles);
        rc = h->dstats.ensure(grid, true, "internal: the Drude statistics' grid exceeds its rows"); if (rc) return rc;
        if (h->d.precision == TGNH_PREC_MIXED && !h->bound.posq_corr) return fail(TGNH_ERR_STATE, "internal: mixed precision without a position correction");
        const int* partner = nullptr;
        rc = device_partner_table(h, &partner); if (rc) return rc;
        {
            Timed t(h, s, KID_OTHER);
            HIP_OK(launch_drude_stats(h->d.precision, h->bound.posq, h->bound.posq_corr, partner, h->d.num_particles, threshold, hist_max,
                                      h->dstats.d_rows, grid, s));
        }
        HIP_OK(hipMemcpyAsync(&r, h->dstats.d_rows + grid, sizeof(r), hipMemcpyDeviceToHost, s));
    }
    rc = finish_query(h, s); if (rc) return rc;
    double max_d2;
    std::memcpy(&max_d2, &r.max_key, sizeof(max_d2));
    out->worst_particle = r.worst == 0x7fffffff ? -1 : r.worst;
    out->pairs = r.pairs; out->over = r.over;
    out->max_distance = r.worst == 0x7fffffff ? 0.0 : std::sqrt(max_d2);
    out->sum_d2 = r.sum_d2;
    std::copy(r.dipole, r.dipole + 3, out->dipole);
    std::copy(r.hist, r.hist + TGNH_DRUDE_HIST_BINS + 1, out->hist);
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// timing / roofline bookkeeping
// ---------------------------------------------------------------------------
static void drain_events(tgnh_handle h) {
    for (size_t i = 0; i < h->timing.ev_used; i++) {
        auto& e = h->timing.ev_pool[i];
        if (hipEventSynchronize(e.b) != hipSuccess) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { h->timing.t_total[e.kid] += ms; h->timing.t_count[e.kid] += 1; }
    }
    h->timing.ev_used = 0;
}
extern "C" tgnh_status tgnh_timing_enable(tgnh_handle h, int on) {
    CHECK_H(h);
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle");
    HIP_OK(hipSetDevice(h->device));
    if (!on) drain_events(h);
    else {
        for (int k = 0; k < KID_COUNT; k++) { h->timing.t_total[k] = 0; h->timing.t_count[k] = 0; }
        h->timing.ev_used = 0;
        while (h->timing.ev_pool.size() < 2048) {        // created here, not lazily inside somebody's timed region
            tgnh_context::Timing::Ev e; e.kid = 0;
            if (hipEventCreate(&e.a) != hipSuccess) break;
            if (hipEventCreate(&e.b) != hipSuccess) { (void)hipEventDestroy(e.a); break; }
            h->timing.ev_pool.push_back(e);
        }
    }
    h->timing.on = on != 0;
    h->timing.only = on >= 2 ? on - 2 : -1;   // on = 2 + kernel id: time that kernel only (2 events per step, not 8)
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_timing_read(tgnh_handle h, int kernel, double* total_ms, int64_t* launches) {
    CHECK_H(h);
    if (kernel < 0 || kernel >= KID_COUNT) return fail(TGNH_ERR_ARG, "bad kernel id");
    if (!h->host_only) { HIP_OK(hipSetDevice(h->device)); drain_events(h); }
    if (total_ms) *total_ms = h->timing.t_total[kernel];
    if (launches) *launches = h->timing.t_count[kernel];
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_algorithmic_bytes(tgnh_handle h, int kernel, double* bytes) {
    CHECK_H(h);
    if (!bytes) return fail(TGNH_ERR_ARG, "null out");
    // state arrays only.  V = velocity vec4, F = 3 x int64, X = position (+correction) per direction.
    const double N = h->d.num_particles;
    const double V = h->d.precision == TGNH_PREC_SINGLE ? 16 : 32;
    const double F = 24;
    const double X = h->d.precision == TGNH_PREC_SINGLE ? 16 : 32;   // mixed: 16 posq + 16 correction; double: 32
    double b = 0;
    switch (kernel) {
        case KID_SKD: b = N * (2 * V + F + 2 * X); break;       // scale+kick+drift: V r/w, F r, X r/w
        case KID_KICK_KE: b = N * (V + F); break;               // kick+KE: V r, F r -- the kicked velocities feed the sums only (every fused structure since round 4)
        case KID_SCALE: b = N * (2 * V + (h->owed.end_folded ? F : 0)); break;    // rescale: V r/w (+ F r where it forms the kicked velocities again)
        case KID_KE: b = N * V; break;                          // KE: V r
        case KID_FORCE: b = N * (X + F); break;                 // harness: X r, F w (x0 excluded)
        case KID_STEP:       // step_kernel: its two passes.  Deferred: (V r, F r) + (V r/w, F r, X r/w); the reference's pass
                             // structure: begin (V r) + (V r/w, F r, X r/w) and end (V r, F r) + (V r/w, F r), averaged per launch
                             // (velocities in the library's planes, owed.planes_live: x, y, z without the 1/m word -- three quarters of V)
            b = (h->d.flags & TGNH_FLAG_DEFER_SCALE) ? N * (3 * (h->owed.planes_live ? 0.75 * V : V) + 2 * F + 2 * X) : N * (6 * V + 3 * F + 2 * X) / 2; break;
        default: b = 0;
    }
    *bytes = b;
    return TGNH_OK;
}
