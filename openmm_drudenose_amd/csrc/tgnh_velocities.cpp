// tgnh_velocities.cpp -- what a caller does to the bound velocities beside the step: the draw (tgnh_set_velocities_to_temperature),
// centre-of-mass motion (tgnh_get_momentum, tgnh_shift_velocities, tgnh_remove_cm_motion, ..._removal) and velocity rescaling
#include "tgnh_host.h"

// Context::setVelocitiesToTemperature (include/drude_tgnh.h has the contract; tgnh_velinit.hip the kernel).  A setVelocities:
// tgnh_state_changed's refusal and its effect come first, then one launch by global index whatever path the handle steps on.
extern "C" tgnh_status tgnh_set_velocities_to_temperature(tgnh_handle h, double temperature, double drude_temperature,
                                                          uint64_t seed, int64_t first_particle, void* stream) {
    CHECK_H(h);
    tgnh_status rc = check_temperatures(temperature, drude_temperature); if (rc) return rc;
    if (first_particle < 0) return fail(TGNH_ERR_ARG, "tgnh_set_velocities_to_temperature: negative first_particle");
    rc = entry(h, true); if (rc) return rc;                     // (buffers bound, not a host-only handle)
    rc = tgnh_state_changed(h); if (rc) return rc;
    const int* partner = nullptr;
    rc = device_partner_table(h, &partner); if (rc) return rc;
    Timed t(h, (hipStream_t)stream, KID_OTHER);
    HIP_OK(launch_velinit(h->d.precision, h->bound.velm, partner, h->d.num_particles, h->d.kB * temperature, h->d.kB * drude_temperature,
                          (unsigned long long)seed, (long long)first_particle, (hipStream_t)stream));
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// centre-of-mass motion (include/drude_tgnh.h has the contract; tgnh_cm_motion.hip the kernels)
// ---------------------------------------------------------------------------
static tgnh_status cm_scratch(tgnh_handle h) {                   // (not cleared: every row is written by the pass before anybody reads it)
    return h->cmm.ensure(index_grid(h->d.num_particles), false, "internal: the momentum pass's grid exceeds its rows");
}
static tgnh_status cm_momentum_launches(tgnh_handle h, hipStream_t s, CmRow** result) {       // pass + row sum of the bound velm -> *result (device)
    tgnh_status rc = cm_scratch(h); if (rc) return rc;
    const int grid = index_grid(h->d.num_particles);
    HIP_OK(launch_cm_momentum(h->d.precision, h->bound.velm, h->d.num_particles, h->cmm.d_rows, grid, s));
    *result = h->cmm.d_rows + grid;
    return TGNH_OK;
}

// momentum pass, row sum, the ranks' four sums added in place where an all-reduce is set (a caller's hook or the library's own
// RCCL, which is installed as that hook), shift.  Nothing here waits for the device.  The caller has seen to tgnh_state_changed.
static tgnh_status cm_removal_launches(tgnh_handle h, hipStream_t s) {
    if (h->xchg.on) return fail(TGNH_ERR_UNSUPPORTED, "centre-of-mass removal with a mailbox exchange attached: the mailboxes carry the kinetic-energy sums only "
                                                      "(tgnh_get_momentum on every rank, add the sums, tgnh_shift_velocities with the same dv everywhere)");
    CmRow* sums = nullptr;
    Timed t(h, s, KID_OTHER);
    tgnh_status rc = cm_momentum_launches(h, s, &sums); if (rc) return rc;
    rc = allreduce_doubles(h, &sums->mass, 4, s); if (rc) return rc;
    HIP_OK(launch_cm_shift(h->d.precision, h->bound.velm, h->d.num_particles, &sums->mass, nullptr, index_grid(h->d.num_particles), s));
    return TGNH_OK;
}

// tgnh_set_cm_motion_removal: before the step whose number is a multiple of `every`, and before that step's own first launch.
// Such a handle never lags (the setter refuses DEFER_SCALE), so tgnh_state_changed's effect is all there is to do.
tgnh_status cm_removal_due(tgnh_handle h, hipStream_t s) {
    if (h->cmm.every <= 0 || h->run.step_count % h->cmm.every != 0) return TGNH_OK;
    h->owed.ke_carry = false;
    return cm_removal_launches(h, s);
}

extern "C" tgnh_status tgnh_remove_cm_motion(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;           // (buffers bound, not a host-only handle, no failure seen before)
    rc = tgnh_state_changed(h); if (rc) return rc;              // (first: refused between the steps of a deferred sequence, and then nothing is written)
    return cm_removal_launches(h, (hipStream_t)stream);
}

extern "C" tgnh_status tgnh_shift_velocities(tgnh_handle h, const double dv[3], void* stream) {
    CHECK_H(h);
    if (!dv) return fail(TGNH_ERR_ARG, "tgnh_shift_velocities: null dv");
    if (!std::isfinite(dv[0]) || !std::isfinite(dv[1]) || !std::isfinite(dv[2])) return fail(TGNH_ERR_ARG, "tgnh_shift_velocities: dv is not finite");
    tgnh_status rc = entry(h, true); if (rc) return rc;
    rc = tgnh_state_changed(h); if (rc) return rc;
    Timed t(h, (hipStream_t)stream, KID_OTHER);
    HIP_OK(launch_cm_shift(h->d.precision, h->bound.velm, h->d.num_particles, nullptr, dv, index_grid(h->d.num_particles), (hipStream_t)stream));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_cm_motion_removal(tgnh_handle h, int every) {
    CHECK_H(h);
    if (every < 0) return fail(TGNH_ERR_ARG, "tgnh_set_cm_motion_removal: negative interval");
    if (every > 0) {
        if (h->d.flags & TGNH_FLAG_DEFER_SCALE)
            return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_cm_motion_removal: velocities lag between the steps of a TGNH_FLAG_DEFER_SCALE handle");
        if (h->xchg.on) return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_cm_motion_removal: a mailbox exchange is attached (it carries the kinetic-energy sums only)");
        if (!h->host_only) {                                    // the scratch now: the first removal may be enqueued inside a stream capture
            HIP_OK(hipSetDevice(h->device));
            tgnh_status rc = cm_scratch(h); if (rc) return rc;
        }
    }
    h->cmm.every = every;
    return TGNH_OK;
}

// Total mass and momentum of this handle's slots (include/drude_tgnh.h has the contract; tgnh_cm_motion.hip the kernels).  A query
// of the velocities, so what a step has left owed to velm is applied first, as tgnh_get_kinetic_energy does; the sweep direction is
// left as it was found.
extern "C" tgnh_status tgnh_get_momentum(tgnh_handle h, void* stream, tgnh_momentum* out) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    if (out->struct_size != sizeof(tgnh_momentum)) return fail(TGNH_ERR_ARG, "tgnh_momentum size mismatch (ABI)");
    tgnh_status rc = entry(h, true); if (rc) return rc;          // (buffers bound, not a host-only handle, no failure seen before)
    hipStream_t s = (hipStream_t)stream;
    const int dir = h->run.sweep_reverse;
    rc = flush_impl(h, s);
    h->run.sweep_reverse = dir;
    if (rc) return rc;
    CmRow& r = h->cmm.h_row;                                     // (the handle's: a copy still in flight when an error returns lands in live memory)
    r = CmRow{};
    CmRow* sums = nullptr;
    {
        Timed t(h, s, KID_OTHER);
        rc = cm_momentum_launches(h, s, &sums); if (rc) return rc;
    }
    HIP_OK(hipMemcpyAsync(&r, sums, sizeof(r), hipMemcpyDeviceToHost, s));
    rc = finish_query(h, s); if (rc) return rc;
    out->reserved = 0;
    out->massive = r.massive; out->mass = r.mass;
    std::copy(r.p, r.p + 3, out->momentum);
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// velocity rescaling (include/drude_tgnh.h has the contract; tgnh_rescale.hip the two small kernels; the rescale is run_tile's)
// ---------------------------------------------------------------------------
static tgnh_status rescale_scratch(tgnh_handle h) {
    if (!h->resc.d_buf) HIP_OK(h->resc.d_buf.alloc(2 * (size_t)h->thermo.L.NT, true));
    return TGNH_OK;
}
static double* rescale_factors(tgnh_handle h) { return h->resc.d_buf; }
static double* rescale_targets(tgnh_handle h) { return h->resc.d_buf + h->thermo.L.NT; }

// A6 with the factors in the scratch: the step's own rescale launch, told where its factors lie (so no chain is adopted and the
// thermostat block is neither read nor written).  Molecules longer than a tile: the launch reads their centre-of-mass velocities
// from a table -- of the velocities as they are (table_fresh: the kinetic-energy pass just before has left it) -- and the table is
// made again of what the launch stored, as flush_impl does.  The gather path computes its own table inside run_gather unless a
// kinetic-energy pass has left it since entry().  The sweep direction is left as it was found.
static tgnh_status rescale_apply(tgnh_handle h, hipStream_t s, bool table_fresh) {
    const int dir = h->run.sweep_reverse;
    tgnh_status rc = big_com_on(h) && !table_fresh ? run_big_com(h, false, s) : TGNH_OK;
    if (!rc) rc = run_tile(h, OP_SCALE, KID_SCALE, s, rescale_factors(h));
    if (!rc && big_com_on(h)) rc = run_big_com(h, false, s);
    h->run.sweep_reverse = dir;
    if (!rc) h->resc.applied = true;
    return rc;
}

static tgnh_status rescale_mailbox_refusal() {
    return fail(TGNH_ERR_UNSUPPORTED, "velocity rescaling to a temperature with a mailbox exchange attached: the mailboxes carry the step's own kinetic-energy sums only "
                                      "(tgnh_compute_kinetic_energies on every rank, form the factors, tgnh_scale_velocities with the same factors everywhere)");
}

// the kinetic-energy pass, its row sum [+ all-reduce], the factors, A6.  Nothing here waits for the device.  The caller has seen
// to tgnh_state_changed (so nothing is owed to velm, and no chain waits for a rescale launch: materialize_chain commits a staged
// block at the most) and to the scratch.
static tgnh_status rescale_to_temperature_launches(tgnh_handle h, double temperature, double drude_temperature, hipStream_t s) {
    if (h->xchg.on) return rescale_mailbox_refusal();
    const ChainLayout& L = h->thermo.L;
    std::vector<double> target = thermostat_nkt(h, h->d.kB * temperature, h->d.kB * drude_temperature);
    for (int k = 0; k < L.NT; k++) if (h->thermo.dof[k] == 0.0) target[k] = RESCALE_INERT;     // (N kT = 0 at any temperature)
    HIP_OK(launch_rescale_put(rescale_targets(h), target.data(), L.NT, s));
    const int dir = h->run.sweep_reverse;
    tgnh_status rc = ke_query_launches(h, s);
    h->run.sweep_reverse = dir;
    if (rc) return rc;
    {
        Timed t(h, s, KID_OTHER);
        HIP_OK(launch_rescale_factors(h->thermo.d_state + L.off_ke_red, rescale_targets(h), L.NT, rescale_factors(h), h->status.d_word, s));
    }
    return rescale_apply(h, s, true);
}

// tgnh_set_velocity_rescaling: placed as cm_removal_due is, and after it
tgnh_status rescale_due(tgnh_handle h, hipStream_t s) {
    if (h->resc.every <= 0 || h->run.step_count % h->resc.every != 0) return TGNH_OK;
    h->owed.ke_carry = false;
    return rescale_to_temperature_launches(h, h->resc.temperature, h->resc.drude_temperature, s);
}

extern "C" tgnh_status tgnh_scale_velocities(tgnh_handle h, const double* factors, int count, void* stream) {
    CHECK_H(h);
    const int NT = h->thermo.L.NT;
    if (!factors) return fail(TGNH_ERR_ARG, "tgnh_scale_velocities: null factors");
    if (count != NT) return fail(TGNH_ERR_ARG, "tgnh_scale_velocities: count is not the number of thermostats (tgnh_get_num_thermostats)");
    std::vector<double> f(factors, factors + NT);
    if (h->d.mode == TGNH_MODE_DUALNH) f[1] = 1.0;              // (dualNH's unused entry: whatever it holds)
    for (double v : f) if (!(v >= 0) || !std::isfinite(v)) return fail(TGNH_ERR_ARG, "tgnh_scale_velocities: a factor is negative or not finite");
    tgnh_status rc = entry(h, true); if (rc) return rc;           // (buffers bound, not a host-only handle, no failure seen before)
    rc = tgnh_state_changed(h); if (rc) return rc;              // (first: refused between the steps of a deferred sequence, and then nothing is written)
    hipStream_t s = (hipStream_t)stream;
    rc = rescale_scratch(h); if (rc) return rc;
    HIP_OK(launch_rescale_put(rescale_factors(h), f.data(), NT, s));    // (by value, with the launch: the caller's array is free again)
    return rescale_apply(h, s, false);
}

extern "C" tgnh_status tgnh_rescale_to_temperature(tgnh_handle h, double temperature, double drude_temperature, void* stream) {
    CHECK_H(h);
    tgnh_status rc = check_temperatures(temperature, drude_temperature); if (rc) return rc;
    rc = entry(h, true); if (rc) return rc;
    if (h->xchg.on) return rescale_mailbox_refusal();           // (before anything of the handle changes)
    rc = tgnh_state_changed(h); if (rc) return rc;
    rc = rescale_scratch(h); if (rc) return rc;
    return rescale_to_temperature_launches(h, temperature, drude_temperature, (hipStream_t)stream);
}

extern "C" tgnh_status tgnh_get_rescale_factors(tgnh_handle h, void* stream, double* factors) {
    CHECK_H(h);
    if (!factors) return fail(TGNH_ERR_ARG, "null out");
    tgnh_status rc = entry(h, true); if (rc) return rc;
    if (!h->resc.applied) return fail(TGNH_ERR_STATE, "tgnh_get_rescale_factors: neither tgnh_scale_velocities nor tgnh_rescale_to_temperature has run on this handle");
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(factors, rescale_factors(h), sizeof(double) * h->thermo.L.NT, hipMemcpyDeviceToHost, s));
    return finish_query(h, s);
}

extern "C" tgnh_status tgnh_set_velocity_rescaling(tgnh_handle h, int every, double temperature, double drude_temperature) {
    CHECK_H(h);
    if (every < 0) return fail(TGNH_ERR_ARG, "tgnh_set_velocity_rescaling: negative interval");
    tgnh_status rc = check_temperatures(temperature, drude_temperature); if (rc) return rc;
    if (every > 0) {
        if (h->d.flags & TGNH_FLAG_DEFER_SCALE)
            return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_velocity_rescaling: velocities lag between the steps of a TGNH_FLAG_DEFER_SCALE handle");
        if (h->xchg.on) return fail(TGNH_ERR_UNSUPPORTED, "tgnh_set_velocity_rescaling: a mailbox exchange is attached (it carries the step's own kinetic-energy sums only)");
        if (!h->host_only) {                                    // the scratch now: the first rescale may be enqueued inside a stream capture
            HIP_OK(hipSetDevice(h->device));
            rc = rescale_scratch(h); if (rc) return rc;
        }
    }
    h->resc.every = every; h->resc.temperature = temperature; h->resc.drude_temperature = drude_temperature;
    return TGNH_OK;
}
