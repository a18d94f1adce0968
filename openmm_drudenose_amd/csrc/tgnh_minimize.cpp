// tgnh_minimize.cpp -- tgnh_minimize_begin / _iterate / _end, tgnh_get_minimize_state and tgnh_run_harness_minimize: the argument
// checks, the mask of moving slots, the launches of one FIRE iteration with the all-reduce between them, and the refusals
// (tgnh_minimize.hip has the kernels; include/drude_tgnh.h the contract)
#include "tgnh_host.h"

static tgnh_status check_desc(const tgnh_minimize_desc* d) {
    const double v[8] = {d->tolerance, d->dt_start, d->dt_max, d->max_step, d->f_inc, d->f_dec, d->alpha_start, d->f_alpha};
    for (double x : v)
        if (!std::isfinite(x)) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: a parameter is not finite");
    if (d->tolerance < 0.0) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: tolerance is negative");
    if (!(d->dt_start > 0.0) || d->dt_max < d->dt_start) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: 0 < dt_start <= dt_max is required");
    if (!(d->max_step > 0.0)) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: max_step must be positive");
    if (d->f_inc < 1.0) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: f_inc must be >= 1");
    if (!(d->f_dec > 0.0 && d->f_dec < 1.0) || !(d->f_alpha > 0.0 && d->f_alpha < 1.0))
        return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: f_dec and f_alpha must lie in (0, 1)");
    if (!(d->alpha_start > 0.0 && d->alpha_start <= 1.0)) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: alpha_start must lie in (0, 1]");
    if (d->n_min < 0) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: n_min is negative");
    if (d->flags & ~TGNH_MIN_DRUDE_ONLY) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: unknown flag bits");
    return TGNH_OK;
}

// what begin and iterate both refuse, positions untouched
static tgnh_status refusals(tgnh_handle h, const char* what) {
    if (h->xchg.on)
        return fail(TGNH_ERR_UNSUPPORTED, std::string(what) + ": a mailbox exchange is attached (it carries the kinetic-energy sums only; the minimiser's "
                                          "four sums go through tgnh_set_allreduce or the library's RCCL)");
    // bits 0 and 2 of tgnh_get_pending_state: a half kick is still owed to velm, from the forces the minimiser is about to replace
    if (h->owed.end_pending || h->owed.kick_pending)
        return fail(TGNH_ERR_STATE, std::string(what) + ": a half kick of the last step is still owed to the velocities (tgnh_flush first)");
    return TGNH_OK;
}

static MinArgs min_args(tgnh_handle h) {
    MinArgs a{};
    a.posq = h->bound.posq; a.corr = h->bound.posq_corr;
    a.force = reinterpret_cast<const long long*>(h->bound.force);
    a.work = h->minim.work; a.mask = h->minim.d_mask;
    a.n = h->d.num_particles; a.padded = h->d.padded_num_particles;
    a.rows = h->minim.d_rows; a.state = h->minim.d_state;
    return a;
}

extern "C" tgnh_status tgnh_minimize_begin(tgnh_handle h, const tgnh_minimize_desc* desc, double* work, void* stream) {
    CHECK_H(h);
    if (!desc || !work) return fail(TGNH_ERR_ARG, "tgnh_minimize_begin: null desc or work");
    tgnh_status rc = check_desc(desc); if (rc) return rc;
    rc = entry(h, true); if (rc) return rc;                       // (buffers bound, not a host-only handle, no failure seen before)
    if (!h->bound.posq || !h->bound.force) return fail(TGNH_ERR_STATE, "tgnh_minimize_begin: positions or forces are not bound");
    rc = refusals(h, "tgnh_minimize_begin"); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stream_capturing(s))
        return fail(TGNH_ERR_STATE, "tgnh_minimize_begin: the stream is capturing (begin uploads the mask and the state block: call it outside the "
                                    "capture and record tgnh_minimize_iterate)");
    const int N = h->d.num_particles;
    if (N < 1 || (int)h->topo.mass.size() != N || h->d.padded_num_particles < N) return fail(TGNH_ERR_STATE, "internal: the descriptor does not match the handle");
    // the mask: a mass, the caller's byte, and -- drude only -- a Drude slot
    std::vector<unsigned char> mask((size_t)N, 0);
    if (desc->flags & TGNH_MIN_DRUDE_ONLY) { for (int d : h->topo.pair_drude) mask[d] = 1; }
    else std::fill(mask.begin(), mask.end(), (unsigned char)1);
    int64_t moving = 0;
    for (int i = 0; i < N; i++) {
        if (h->topo.mass[i] == 0.0 || (desc->moving && !desc->moving[i])) mask[i] = 0;
        moving += mask[i];
    }
    if (moving == 0) return fail(TGNH_ERR_STATE, "tgnh_minimize_begin: no slot moves (every slot is massless, masked out, or no Drude particle)");
    tgnh_context::Minimize& m = h->minim;
    m.drop();                                                     // (a begin without an end: the earlier minimisation's buffers go)
    const int grid = index_grid(N);
    HIP_OK(m.d_mask.alloc((size_t)N));
    HIP_OK(m.d_rows.alloc(4 * ((size_t)grid + 1)));               // (every row is written by the pass before anybody reads it)
    HIP_OK(m.d_state.alloc(1));
    MinState& st = m.h_state;
    st = MinState{};
    st.dt = desc->dt_start; st.alpha = desc->alpha_start; st.n_min = desc->n_min;
    st.tolerance = desc->tolerance; st.dt_max = desc->dt_max; st.max_step = desc->max_step;
    st.f_inc = desc->f_inc; st.f_dec = desc->f_dec; st.alpha_start = desc->alpha_start; st.f_alpha = desc->f_alpha;
    HIP_OK(hipMemcpyAsync(m.d_mask, mask.data(), (size_t)N, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(m.d_state, &st, sizeof(MinState), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(work, 0, sizeof(double) * 3 * (size_t)N, s));
    HIP_OK(hipStreamSynchronize(s));                              // (the mask is this call's: it has left before the call returns)
    m.work = work; m.moving = moving; m.active = true;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_minimize_iterate(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    tgnh_context::Minimize& m = h->minim;
    if (!m.active) return fail(TGNH_ERR_STATE, "tgnh_minimize_iterate: no minimisation is under way (tgnh_minimize_begin first)");
    rc = refusals(h, "tgnh_minimize_iterate"); if (rc) return rc;
    if (!m.d_mask || !m.d_rows || !m.d_state || !m.work || !h->bound.posq || !h->bound.force)
        return fail(TGNH_ERR_STATE, "internal: the minimiser's buffers are not all there");
    hipStream_t s = (hipStream_t)stream;
    const MinArgs a = min_args(h);
    const int grid = index_grid(a.n);
    const bool hook = h->xchg.allreduce != nullptr;
    Timed t(h, s, KID_OTHER);
    HIP_OK(launch_min_sums(a, grid, hook ? 0 : 1, s));
    if (hook) {                                                   // {P, FF, VV, moving} of every rank, added in place, in one call
        rc = allreduce_doubles(h, a.rows + 4 * (size_t)grid, 4, s); if (rc) return rc;
        HIP_OK(launch_min_decide(a, grid, s));
    }
    HIP_OK(launch_min_update(h->d.precision, a, grid, s));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_minimize_state(tgnh_handle h, void* stream, tgnh_minimize_state* out) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "tgnh_get_minimize_state: null out");
    tgnh_status rc = entry(h, true); if (rc) return rc;
    tgnh_context::Minimize& m = h->minim;
    if (!m.active || !m.d_state) return fail(TGNH_ERR_STATE, "tgnh_get_minimize_state: no minimisation is under way (tgnh_minimize_begin first)");
    hipStream_t s = (hipStream_t)stream;
    MinState& st = m.h_state;                                     // (the handle's: a copy still in flight when an error returns lands in live memory)
    HIP_OK(hipMemcpyAsync(&st, m.d_state, sizeof(MinState), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    tgnh_minimize_state r{};
    r.iterations = st.iterations; r.uphill = st.uphill; r.since_uphill = st.since_uphill; r.moving = m.moving;
    r.converged = st.converged;
    r.dt = st.dt; r.alpha = st.alpha; r.power = st.sums[0]; r.ff = st.sums[1]; r.vv = st.sums[2]; r.rms_force = st.rms;
    *out = r;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_minimize_end(tgnh_handle h) {
    CHECK_H(h);
    if (!h->host_only && h->minim.d_mask) HIP_OK(hipSetDevice(h->device));      // (device memory is released on the handle's device)
    h->minim.drop();
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_run_harness_minimize(tgnh_handle h, const void* x0, double k_drude, double k_tether, int iterations, void* stream) {
    CHECK_H(h);
    if (iterations < 0) return fail(TGNH_ERR_ARG, "tgnh_run_harness_minimize: negative iteration count");
    if (!h->minim.active) return fail(TGNH_ERR_STATE, "tgnh_run_harness_minimize: no minimisation is under way (tgnh_minimize_begin first)");
    for (int i = 0; i < iterations; i++) {
        tgnh_status rc = tgnh_harness_force(h, x0, k_drude, k_tether, const_cast<void*>(h->bound.force), stream); if (rc) return rc;
        rc = tgnh_minimize_iterate(h, stream); if (rc) return rc;
    }
    return TGNH_OK;
}
