// tgnh_host.h -- what the host units behind the C ABI (include/drude_tgnh.h) share: tgnh_topology.cpp, tgnh_lifecycle.cpp,
// tgnh_exchange.cpp, tgnh_step.cpp, tgnh_velocities.cpp, tgnh_queries.cpp, tgnh_positions.cpp, tgnh_frames.cpp, tgnh_minimize.cpp, tgnh_constraints.cpp, tgnh_virtual_sites.cpp, tgnh_drude_force.cpp, tgnh_bonded.cpp, tgnh_nonbonded.cpp, tgnh_ewald.cpp, tgnh_pme.cpp, tgnh_harness_host.cpp (each says at its top what it holds).  Kernels
// live in tgnh_kernels.hip (tgnh_tile_kernels.h, tgnh_wave_kernels.h, tgnh_chain_kernels.h), tgnh_gather.hip, tgnh_velinit.hip,
// tgnh_drude_stats.hip, tgnh_cm_motion.hip, tgnh_rescale.hip, tgnh_scale_positions.hip, tgnh_wrap.hip, tgnh_minimize.hip, tgnh_constraints.hip, tgnh_virtual_sites.hip, tgnh_drude_force.hip, tgnh_bonded.hip, tgnh_nonbonded.hip, tgnh_ewald.hip, tgnh_pme.hip, tgnh_vplanes.hip and tgnh_harness.hip.
// The library's forces (virtual sites, DrudeForce, bonded, the nonbonded exceptions) share one form, said once: the table of receiving
// slots and its inversion in tgnh_receivers.h, its owner in tgnh_context.h (Receivers), the lane's loop in tgnh_receiver_device.h.
//
// Reference semantics followed (scychon/openmm_drudeNose):
//   Ref = platforms/reference/src/ReferenceDrudeTGNHKernels.cpp
//   Cu  = platforms/cuda/src/CudaDrudeTGNHKernels.cpp
//   API = openmmapi/src/DrudeTGNHIntegrator.cpp
#ifndef TGNH_HOST_H_
#define TGNH_HOST_H_

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tgnh_context.h"
#include "tgnh_minimize.h"
#include "tgnh_rescale.h"
#include "tgnh_scale_positions.h"
#include "tgnh_vplanes.h"

using namespace tgnh;

#pragma GCC visibility push(hidden)      // shared between the units, not with the world
inline tgnh_status fail(tgnh_status code, const std::string& msg) {
    tgnh_set_error(msg);
    return code;
}
#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(TGNH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define CHECK_H(h) do { if (!(h)) return fail(TGNH_ERR_ARG, "null handle"); } while (0)

// what a description says about its handle, for every unit that asks
inline bool com_thermostat_on(const tgnh_desc& d) { return d.mode == TGNH_MODE_TGNH && d.use_com_temp_group; }
inline int pass_kind(const tgnh_desc& d) { return (d.flags & TGNH_FLAG_DEFER_SCALE) ? 0 : 1; }   // step_kernel's kind of the pass structure: 0 a whole deferred step, 1 the reference's halves
// tgnh_topology.cpp
void make_layout(tgnh_context* c);
tgnh_status build_topology(tgnh_context* c, const tgnh_desc* d);
void local_dof_terms(tgnh_context* c);
tgnh_status check_temperatures(double temperature, double drude_temperature);
void set_bath_temperatures(tgnh_context* c, double temperature, double drude_temperature);
std::vector<double> thermostat_nkt(const tgnh_context* c, double realkbT, double drudekbT);   // N kT per thermostat at these kT (stores nothing)
void thermostat_targets(tgnh_context* c, std::vector<double>& st);
tgnh_status finalize_thermostat(tgnh_context* c);
std::vector<int> partner_table(const tgnh_context* c);
tgnh_status device_partner_table(tgnh_context* c, const int** out);
// tgnh_lifecycle.cpp
tgnh_status deferred_guard(tgnh_handle h, const char* what);
// tgnh_step.cpp
void note_status(tgnh_handle h, uint32_t flags);
tgnh_status entry(tgnh_handle h, bool need_bufs);
bool stream_capturing(hipStream_t s);                          // a stream capture is recording s: nothing synchronous may be done on it
tgnh_status finish_query(tgnh_handle h, hipStream_t s);        // a query's tail: the status word behind what it enqueued, wait, the sticky failure
tgnh_status allreduce_doubles(tgnh_handle h, double* device_ptr, int count, hipStream_t s);   // the hook on these sums, in place (TGNH_OK: none is set)
bool resident_now(tgnh_handle h);
tgnh_status allreduce_hook(tgnh_handle h, hipStream_t s);      // ... on the summed kinetic energies
bool big_com_on(tgnh_handle h);
tgnh_status run_big_com(tgnh_handle h, bool kick, hipStream_t s);
tgnh_status run_tile(tgnh_handle h, int ops, int kid, hipStream_t s, const double* scale = nullptr);
GatherArgs gather_args(tgnh_handle h, const double* scale);
ChainArgs chain_args(tgnh_handle h);
tgnh_status run_chain_gather(tgnh_handle h, hipStream_t s, bool sum_only);
tgnh_status materialize_chain(tgnh_handle h, hipStream_t s);
tgnh_status settle_kick(tgnh_handle h, hipStream_t s);
tgnh_status settle_end(tgnh_handle h, hipStream_t s);
tgnh_status velm_current(tgnh_handle h, hipStream_t s);        // velocity planes left live with nothing else pending go back to velm (before velm is touched without a settle)
tgnh_status flush_impl(tgnh_handle h, hipStream_t s);
tgnh_status ke_query_launches(tgnh_handle h, hipStream_t s);    // tgnh_queries.cpp: what tgnh_compute_kinetic_energies enqueues behind its entry checks
tgnh_status cm_removal_due(tgnh_handle h, hipStream_t s);      // tgnh_velocities.cpp: tgnh_set_cm_motion_removal's launches where this step is due; a step begins with this
tgnh_status rescale_due(tgnh_handle h, hipStream_t s);         // ... and then with tgnh_set_velocity_rescaling's
// tgnh_ewald.cpp: what tgnh_set_nonbonded_ewald and tgnh_set_nonbonded_pme share
tgnh_status ewald_set_begin(tgnh_handle h, const char* me, bool clear, bool* done);       // the capture refusal, the clearing call, the table that must be in force
void ewald_set_constants(tgnh_context::Ewald& e, double alpha);                           // on, alpha, tsp, a4
tgnh_status ewald_set_shared(tgnh_handle h, tgnh_context::Ewald& e);                      // E_self, bgn, the exclusion rows and their receiver table, misc, totals
// tgnh_pme.cpp: tgnh_compute_nonbonded_force's launches with particle-mesh Ewald on; L the edges of the call's box
tgnh_status pme_launches(tgnh_handle h, const double L[3], void* force, int want_energy, hipStream_t s);
// tgnh_positions.cpp
tgnh_status molecules_ensure(tgnh_context* c, const char* what);              // the table in force: the caller's, or the default resolved now (TGNH_ERR_STATE: no resid)
tgnh_status molecules_launch_bounds(const tgnh_context* c);                   // what the launches over the table are bound by, against what the tables hold
tgnh_status molecules_device(tgnh_context* c, hipStream_t s);                 // the molecule table's device copies, made once per table (never inside a capture)

// a launch between two events when timing is on (tgnh_timing_enable)
struct Timed {
    tgnh_context* c; hipStream_t s; int kid; tgnh_context::Timing::Ev* ev = nullptr;
    Timed(tgnh_context* c_, hipStream_t s_, int kid_) : c(c_), s(s_), kid(kid_) {
        if (!c->timing.on) return;
        if (c->timing.only >= 0 && kid != c->timing.only) return;
        if (c->timing.ev_used == c->timing.ev_pool.size()) {
            tgnh_context::Timing::Ev e; e.kid = kid;
            if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
            c->timing.ev_pool.push_back(e);
        }
        ev = &c->timing.ev_pool[c->timing.ev_used++];
        ev->kid = kid;
        (void)hipEventRecord(ev->a, s);
    }
    ~Timed() { if (ev) (void)hipEventRecord(ev->b, s); }
};
// What a feature call (constraints, virtual sites, the library's forces) refuses before it launches anything: a host-only handle, a
// handle whose arrays are not bound -- `needs` names the one the call works on -- and, where `sticky`, a failure the device
// reported earlier (tgnh_get_status_flags' rule).
inline tgnh_status feature_ready(tgnh_handle h, const char* what, void* tgnh_context::Bound::*needs, bool sticky) {
    CHECK_H(h);
    if (h->host_only) return fail(TGNH_ERR_STATE, std::string(what) + ": host-only handle (device -1): no GPU work can be launched on it");
    if (!(h->bound.*needs)) return fail(TGNH_ERR_STATE, std::string(what) + ": tgnh_bind_buffers has not been called");
    if (sticky && h->status.failed_code) return fail(h->status.failed_code, h->status.failed);
    return TGNH_OK;
}
// An energy query's tail: the four totals that the one-work-group sum enqueued on s leaves at `totals`, on the host when this returns
inline tgnh_status fetch_totals(tgnh_handle h, const double* totals, hipStream_t s, double (&got)[4]) {
    HIP_OK(hipMemcpyAsync(got, totals, sizeof(got), hipMemcpyDeviceToHost, s));
    return finish_query(h, s);
}
template <typename Row> tgnh_status tgnh::RowScratch<Row>::ensure(int grid, bool zero, const char* too_small) {
    if (!d_rows) {
        HIP_OK(d_rows.alloc((size_t)grid + 1, zero));
        rows_allocated = grid + 1;
    }
    if (grid < 1 || grid > INDEX_GRID_CAP || grid + 1 > rows_allocated) return fail(TGNH_ERR_STATE, too_small);
    return TGNH_OK;
}
#pragma GCC visibility pop

#endif
