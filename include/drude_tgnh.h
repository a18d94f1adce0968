/*
 * drude_tgnh.h -- C ABI of the MI355X (gfx950) DrudeTGNHIntegrator step kernel.
 *
 * This is the drop-in boundary: what an OpenMM-HIP `KernelImpl` for
 * `IntegrateDrudeTGNHStepKernel` (reference: openmmapi/include/openmm/DrudeTGNHKernels.h:48-74)
 * binds to.  Plain C types only; the caller owns the particle buffers (OpenMM's
 * posq / velm / force / posDelta device arrays), the library owns topology,
 * scratch and thermostat state.  All work is enqueued on the caller's HIP
 * stream; functions named *_get_* that return host values synchronise that
 * stream, nothing else does.  One handle per device; handles are not
 * thread-safe.  Every function returns a tgnh_status; tgnh_last_error() has
 * the message (the OpenMM glue turns it into an OpenMMException).
 *
 * Reference interfaces replaced (file:line in scychon/openmm_drudeNose):
 *   tgnh_create            IntegrateDrudeTGNHStepKernel::initialize
 *                          platforms/cuda/src/CudaDrudeTGNHKernels.cpp:75-282,
 *                          platforms/reference/src/ReferenceDrudeTGNHKernels.cpp:104-219
 *   tgnh_step_begin/_end   IntegrateDrudeTGNHStepKernel::execute
 *                          CudaDrudeTGNHKernels.cpp:284-408 split at the force call-out (:380);
 *                          ReferenceDrudeTGNHKernels.cpp:221-415 split at :384
 *   tgnh_get_kinetic_energy  ::computeKineticEnergy  CudaDrudeTGNHKernels.cpp:654-661,
 *                          ReferenceDrudeTGNHKernels.cpp:586-588
 *   tgnh_set_*             values the reference re-reads from the integrator every
 *                          step (CudaDrudeTGNHKernels.cpp:292,298,437-439,469)
 *   tgnh_destroy           ~CudaIntegrateDrudeTGNHStepKernel  CudaDrudeTGNHKernels.cpp:52-73
 */
#ifndef DRUDE_TGNH_H_
#define DRUDE_TGNH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGNH_ABI_VERSION 1

typedef int tgnh_status;
enum {
    TGNH_OK = 0,
    TGNH_ERR_ARG = -1,            /* bad argument / size */
    TGNH_ERR_GROUP_MISMATCH = -2, /* CudaDrudeTGNHKernels.cpp:145-146, :192-193 */
    TGNH_ERR_HARDWALL = -3,       /* ReferenceDrudeTGNHKernels.cpp:311-312 */
    TGNH_ERR_UNSUPPORTED = -4,    /* what the reference itself cannot run (a massless pair member, a molecule without mass under the COM group,
                                     dualNH without a pair), sizes beyond an index's or a bin's reach, a flag the topology cannot take;
                                     NOT a topology the tiles cannot hold: that steps on the gather path (tgnh_get_step_path) */
    TGNH_ERR_HIP = -5,            /* a HIP runtime call failed */
    TGNH_ERR_STATE = -6           /* call order (buffers not bound, ...) */
};

/* Semantic mode: the two platform implementations differ. */
enum { TGNH_MODE_DUALNH = 0,      /* platforms/reference semantics */
       TGNH_MODE_TGNH = 1 };      /* platforms/cuda semantics (temperature groups + COM) */

/* OpenMM precision modes: real = posq type, mixed = velm/posDelta type. */
enum { TGNH_PREC_SINGLE = 0,      /* float4 posq, float4 velm */
       TGNH_PREC_MIXED = 1,       /* float4 posq + float4 posqCorrection, double4 velm */
       TGNH_PREC_DOUBLE = 2 };    /* double4 posq, double4 velm */

/* flags for tgnh_desc.flags */
enum { TGNH_FLAG_DEFER_SCALE = 2 };    /* the end-of-step rescale AND the second half kick are left pending and folded
                                        * into the next step's first pass: between tgnh_step_end and the next
                                        * tgnh_step_begin velm lags and the force buffer must stay as it is; tgnh_flush
                                        * makes velm the reference's end-of-step state.  (1 is reserved.) */
enum { TGNH_FLAG_WAVE_TILES = 8 };     /* run the kinetic-energy passes and the one-launch deferred step over wave tiles (one
                                        * wavefront = <= 64 slots) whenever the topology has them -- every molecule and
                                        * pair inside a wavefront, <= 8 temperature groups -- whatever their fill.  Without the
                                        * flag the library takes them only where they are >= 90 % full (60-slot water tiles: yes;
                                        * 35-slot cations: no, the 512-slot tile kernels are faster there).  Same integrator
                                        * either way. */
enum { TGNH_FLAG_RESIDENT_STEP = 4 };  /* whole thermostat halves in ONE launch whose work-groups meet on the device
                                        * (step_kernel).  Alone: the reference's pass structure, two launches per
                                        * step (KE + chain + rescale, kick, drift | kick + KE + chain + rescale), velocities
                                        * never lag -- usable wherever the plain structure is.  With DEFER_SCALE:
                                        * tgnh_step_end launches nothing and the next tgnh_step_begin runs that end half and
                                        * its own begin half in one launch.  Either way the handle needs the device to itself
                                        * while stepping (see tgnh_set_resident_share); <= 8 temperature groups, no
                                        * collective hook, and chains of 1-4 links with DEFER_SCALE on a topology with wave tiles
                                        * (wstep_kernel; not DUALNH's coupled chain of 2-4 links, useDrudeNHChains = 0), one-link
                                        * chains otherwise (step_kernel) -- else it quietly steps with
                                        * the tile launches (tgnh_get_resident_kernel says which).
                                        * With a mailbox exchange attached and DEFER_SCALE, state queries between steps are
                                        * collective over the ranks. */

enum { TGNH_FLAG_TRUST_STATE_CHANGED = 16 };  /* The reference's pass structure (velocities never lag, no TGNH_FLAG_DEFER_SCALE)
                                        * without the first half step's kinetic-energy pass: after the end half's rescale every bin
                                        * is exactly s^2 times the bin its chain started from, and the chain has tracked that product
                                        * (CudaDrudeTGNHKernels.cpp:574), so the next tgnh_step_begin / _begin_kick starts its chain
                                        * from it -- one launch instead of KE + chain + rescale.  The caller vouches that NOTHING
                                        * writes velm between tgnh_step_end / _end_thermo and the next begin without
                                        * tgnh_state_changed (DrudeTGNHIntegrator.cpp:166-170): setVelocities does call it, OpenMM's
                                        * CMMotionRemover and AndersenThermostat edit velocities in updateContextState without -- the
                                        * glue sets the flag only for a System that holds neither.  Invalidated (the next half
                                        * recomputes) by tgnh_state_changed, tgnh_bind_buffers, tgnh_set_thermostat_state,
                                        * tgnh_set_global_dof_terms, the split entry points that write velocities, attaching an
                                        * exchange; ignored when sharded (hook, RCCL, mailboxes), with DEFER_SCALE, and for a topology
                                        * in which a molecule spans two temperature groups (tgnh_get_pending_state bit 9 shows
                                        * whether the next half will carry over).  A hipGraph of steps recorded while carrying over
                                        * holds no KE pass: replay it only while the promise holds. */

enum { TGNH_FLAG_GATHER = 32 };        /* step on the GATHER path (tgnh_get_step_path) whatever the topology: the reference's own
                                        * un-fused kernels by global index, which the library otherwise takes only for what its
                                        * tiles cannot hold.  For comparisons and as a fallback; several times slower per slot. */

typedef struct tgnh_desc {
    uint32_t struct_size;         /* sizeof(tgnh_desc), ABI check */
    int32_t mode;                 /* TGNH_MODE_* */
    int32_t precision;            /* TGNH_PREC_* */
    int32_t flags;                /* TGNH_FLAG_* ; any other bit: TGNH_ERR_ARG (a binding built against a newer header) */
    int32_t device;               /* HIP device ordinal; -1 = host-only handle (topology, tiles, dof queries; no launches) */
    int32_t num_particles;        /* N: particle slots owned by this handle */
    int32_t padded_num_particles; /* stride of the 3 force planes (OpenMM PADDED_NUM_ATOMS), >= N and <= 715 827 882 (3 x stride in 32-bit indices, as K :318-320) */
    int32_t num_pairs;            /* P: Drude pairs, DrudeForce order */
    int32_t num_groups;           /* G: getNumTempGroups() (TGNH mode) */
    int32_t num_residues;         /* R: getNumResidues()   (TGNH mode) */
    int32_t num_constraints;
    int32_t has_cm_motion_remover;
    const double* mass;           /* [N] System::getParticleMass */
    const int32_t* pair_drude;    /* [P] DrudeForce::getParticleParameters p  */
    const int32_t* pair_parent;   /* [P] DrudeForce::getParticleParameters p1 */
    const int32_t* group;         /* [N] getParticleTempGroup (TGNH mode; ignored in DUALNH -- the Reference platform has no temperature groups -- and may be NULL there) */
    const int32_t* resid;         /* [N] getParticleResId     (TGNH mode; may be NULL in DUALNH) */
    const int32_t* constraint_i;  /* [num_constraints] or NULL */
    const int32_t* constraint_j;
    double kB;                    /* OpenMM BOLTZ, kJ/mol/K */
    double temperature, coupling_time;
    double drude_temperature, drude_coupling_time;
    double step_size;
    int32_t drude_steps_per_real_step;
    int32_t num_nh_chains;
    int32_t use_drude_nh_chains;
    int32_t use_com_temp_group;
    double max_drude_distance;    /* 0 = hard wall off */
} tgnh_desc;

typedef struct tgnh_context* tgnh_handle;

/* What is reproducible bit for bit (no atomics anywhere in a sum; every order of additions is fixed by the topology, the grid
 * and the direction of the sweep):
 *   - the same handle configuration, the same state and the same step counter give the same bits from there on: the sweep
 *     direction, which orders the additions of the kinetic-energy sums, is a function of the step counter, and queries
 *     (tgnh_get_*, tgnh_compute_kinetic_energies, tgnh_flush) neither change it nor anything else of the trajectory -- so a
 *     run restored from a checkpoint (thermostat arrays + tgnh_set_time) continues bit for bit, and a query asked twice
 *     returns the same bits (the plain kinetic energy of tgnh_get_kinetic_energy included);
 *   - the ranks of one sharded run hold bit-identical thermostats whatever each of them is asked in between: every rank adds
 *     the same world x NT sums in rank order (mailboxes) or receives the same all-reduced values (RCCL) and runs the same
 *     chain arithmetic, in the standalone chain kernel or inside a streaming launch;
 *   - different pass structures (flags), grids (devices with another number of compute units) or shardings of the same
 *     system sum in different orders: they agree to rounding (1e-12 over 100 steps), not bit for bit. */

/* Collective hook for particle-sharded runs: in-place sum of `count` doubles
 * at device pointer `buf` over all ranks, enqueued on `stream` (an RCCL
 * ncclAllReduce in the glue / a torch.distributed all_reduce in the harness).
 * Must not synchronise the host. */
typedef int (*tgnh_allreduce_fn)(void* buf, int count, void* stream, void* user);

const char* tgnh_last_error(void);
int tgnh_abi_version(void);

tgnh_status tgnh_create(const tgnh_desc* desc, tgnh_handle* out);
tgnh_status tgnh_destroy(tgnh_handle h);

/* OpenMM device arrays (raw device pointers).  posq_correction only in MIXED
 * mode, pos_delta only for the constrained (split) path; pass NULL otherwise.
 *   posq   real4  [N]  (x,y,z,q)
 *   velm   mixed4 [N]  (vx,vy,vz,1/m)   -- w is read as the inverse mass
 *   force  int64  [3*padded]  fixed point x 2^32, planes x|y|z
 *   pos_delta mixed4 [N]
 * When a pointer differs from the one bound before, what the runtime knows of the allocation behind each pointer is checked
 * against what the launches touch (TGNH_ERR_ARG: a float4 array bound as double4, N for padded).  A call with the five pointers
 * already bound returns at once WITHOUT that check (the glue binds at every step): an array freed and allocated again, smaller,
 * at the same address is the caller's to rebind through a NULL-free change of any pointer, or to not do. */
tgnh_status tgnh_bind_buffers(tgnh_handle h, void* posq, void* posq_correction, void* velm,
                              const void* force, void* pos_delta);

/* Integrator scalars re-read every step by the reference. */
tgnh_status tgnh_set_step_size(tgnh_handle h, double dt);
tgnh_status tgnh_set_drude_steps_per_real_step(tgnh_handle h, int n);
tgnh_status tgnh_set_max_drude_distance(tgnh_handle h, double d);

/* Particle sharding: dof terms are additive over ranks.  terms = per-thermostat
 * degrees of freedom before the global CMMotionRemover correction
 * (NT values, see tgnh_get_num_thermostats).  Sum them over ranks and hand them back. */
tgnh_status tgnh_get_local_dof_terms(tgnh_handle h, double* terms, int* count);
tgnh_status tgnh_set_global_dof_terms(tgnh_handle h, const double* terms, int count);
tgnh_status tgnh_set_allreduce(tgnh_handle h, tgnh_allreduce_fn fn, void* user);

/* The collective done by the library itself: one ncclAllReduce(sum, ncclDouble, NT values, in place) per thermostat half
 * step -- per time step with TGNH_FLAG_DEFER_SCALE -- enqueued on the step's stream between the row sum and the chain
 * (the reference integrates on one device only, platforms/cuda/src/CudaDrudeTGNHKernelFactory.cpp:62: this is the exchange
 * north_star adds, "a single RCCL all-reduce over xGMI of the per-group KE scalars each step").  Either hand over a
 * communicator the caller already has (an ncclComm_t of the RCCL this library is linked against), or let the library make
 * its own: rank 0 calls tgnh_rccl_unique_id and passes the TGNH_RCCL_ID_BYTES to every rank by whatever means the caller
 * has (MPI, a file, torch.distributed), then EVERY rank calls tgnh_rccl_init (collective; the handle's device must be
 * current-able).  Replaces a tgnh_set_allreduce hook; tgnh_rccl_shutdown (or tgnh_destroy) destroys a communicator the
 * library made.  Capturable into a hipGraph like every launch of a step. */
#define TGNH_RCCL_ID_BYTES 128
tgnh_status tgnh_rccl_unique_id(void* id_out);
tgnh_status tgnh_rccl_init(tgnh_handle h, int world, int rank, const void* id);
tgnh_status tgnh_set_rccl_comm(tgnh_handle h, void* nccl_comm);
tgnh_status tgnh_rccl_shutdown(tgnh_handle h);
/* TGNH_FLAG_RESIDENT_STEP: this handle may fill 1/share of the device's resident work-group slots (default 1 = all of
 * them).  Several handles that step concurrently on one device (replicas, or the ranks of a rehearsal on one GPU) must
 * share it, or their launches wait for each other's work-groups until the meeting times out (status bit 3). */
tgnh_status tgnh_set_resident_share(tgnh_handle h, int share);
/* Work-groups of the resident step kernel per compute unit that tgnh_create found resident together (a census launch checks
 * the occupancy query); 0 = the handle steps the DEFER_SCALE way (flag not set, or nothing passed the census).  The count is
 * that of the kernel tgnh_get_resident_kernel names (a handle may have one for step_kernel and a smaller one for wstep_kernel):
 * the one-launch step's grid is min(work to hand out, this count x compute units / resident share). */
tgnh_status tgnh_get_resident_work_groups(tgnh_handle h, int* per_compute_unit);
/* How this handle steps: *gather = 0 the tiled kernels (every Drude partner and molecular centre of mass an on-chip look-up inside
 * a tile of <= 512 consecutive slots, <= 32 temperature groups), 1 the GATHER path -- the reference's own un-fused kernels by
 * global index (drudeTGNH.cu:82-301, 307-365, 435-574: normalParticles / pairParticles / particleResId lists, bins sized G + 2),
 * taken for what the tiles cannot hold: a Drude particle more than a tile from its parent, pairs overlapping so densely in a long
 * molecule that no cut between two of them lies within a tile's reach, more than 32 temperature groups (up to 2046), chains
 * too long for the on-chip forms; 2 the same with its own row sum and chain kernels (more than 34 thermostats).  Much slower per
 * slot (every look-up a global load) and always in the reference's pass structure: TGNH_FLAG_DEFER_SCALE, _RESIDENT_STEP,
 * _TRUST_STATE_CHANGED are ignored on it.  *reason (may be NULL): why, "" for the tiled path; valid until tgnh_destroy.
 * SHARDED RUNS: the ranks exchange once per thermostat half step they run, and a rank on the gather path runs the reference's
 * two halves per step whatever its flags say -- so all ranks must be on the same path: if tgnh_get_step_path reports the gather
 * path on ANY rank (agree on it with the collective at hand), create every rank's handle with TGNH_FLAG_GATHER.  Ranks that
 * disagree wait for exchanges their peers never send: the mailbox exchange times out (status bit 2), a collective hangs. */
tgnh_status tgnh_get_step_path(tgnh_handle h, int* gather, const char** reason);
/* Which kernel this handle's next tgnh_step_begin runs as its one launch: 0 none (the streaming launches), 1 step_kernel (512-slot
 * tiles, one-link chains), 2 wstep_kernel (a whole deferred step over wave tiles, chains of 1-4 links). */
tgnh_status tgnh_get_resident_kernel(tgnh_handle h, int* which);

/* Mailbox exchange: the same all-reduce of the NT kinetic-energy sums, done by the integrator's own kernels with
 * plain stores into every peer's mailbox over xGMI (no collective launch on the step's critical path).  Optional;
 * when attached it replaces the hook above.  One rank per GPU (or several handles in one process):
 *   create  allocates this rank's mailbox and returns its IPC handle (TGNH_XCHG_HANDLE_BYTES, for peers in other
 *           processes) and its device pointer (for peers in this process);
 *   attach  takes every rank's IPC handle, rank-major (own entry ignored) -- or every rank's pointer;
 * then all ranks step in lockstep.  Sums are added in rank order on every rank: bit-identical thermostats.
 * A peer that never answers sets status bit 2 after a bounded wait (tgnh_get_status_flags); nothing hangs.
 * Teardown across processes: every rank detaches (unmaps the peers' mailboxes), then -- after a barrier of the
 * caller's -- destroys its handle (frees its own mailbox). */
#define TGNH_XCHG_HANDLE_BYTES 64
tgnh_status tgnh_exchange_create(tgnh_handle h, int world, int rank, void* ipc_handle_out, void** mailbox_out);
tgnh_status tgnh_exchange_attach(tgnh_handle h, const void* ipc_handles);
tgnh_status tgnh_exchange_attach_pointers(tgnh_handle h, void* const* mailboxes);
tgnh_status tgnh_exchange_detach(tgnh_handle h);
/* How long the waits of the mailbox exchange took on this rank since the last call (or attach): per exchange, the time from
 * "this rank's sums are complete" to "every rank's sums are here" as seen by work-group 0 of the waiting launch, measured on
 * the device (wall_clock64, 10 ns ticks) -- the figure that says WHERE a sharded run loses time when it scales worse than the
 * one-GPU ceiling: a rank that waits long is waiting for a slower peer or for the link.  Synchronises `stream`; resets. */
tgnh_status tgnh_exchange_wait_stats(tgnh_handle h, void* stream, double* mean_us, double* max_us, int64_t* exchanges);

/* One time step, split at the force call-out:
 *   begin: [KE -> chain ->] rescale, half kick, drift, hard wall
 *   (caller: virtual sites, calcForcesAndEnergy)
 *   end:   half kick, KE -> chain -> rescale, time += dt */
tgnh_status tgnh_step_begin(tgnh_handle h, void* stream);
tgnh_status tgnh_step_end(tgnh_handle h, void* stream);
/* Split variants around OpenMM's constraint call-outs (posDelta path):
 *   begin_kick:  [KE -> chain ->] rescale, half kick, posDelta = dt*v        (CudaDrudeTGNHKernels.cpp:336-360)
 *   (caller: applyConstraints on posDelta)
 *   begin_move:  pos += posDelta, v = posDelta/dt, hard wall                 (:366-376)
 *   end_kick:    half kick                                                   (:384-388)
 *   (caller: applyVelocityConstraints)
 *   end_thermo:  KE -> chain -> rescale, time += dt                          (:394-406) */
tgnh_status tgnh_step_begin_kick(tgnh_handle h, void* stream);
tgnh_status tgnh_step_begin_move(tgnh_handle h, void* stream);
tgnh_status tgnh_step_end_kick(tgnh_handle h, void* stream);
tgnh_status tgnh_step_end_thermo(tgnh_handle h, void* stream);
/* Apply the half kick and rescale still pending (TGNH_FLAG_DEFER_SCALE) so velm is the
 * reference's end-of-step state; call before anything else reads OR WRITES velm -- between tgnh_step_begin and tgnh_step_end
 * too on a DEFER_SCALE | RESIDENT_STEP handle, where the velocities may live in the library's own planes (bit 10 of
 * tgnh_get_pending_state) and the flush is what writes them to velm.  Nothing pending: no launch. */
tgnh_status tgnh_flush(tgnh_handle h, void* stream);
/* A caller that captured `nsteps` steps into a hipGraph and replays it tells the handle here: the host-side
 * clock and step count advance only when the step functions are called, not when a graph is replayed.
 * Determinism: the sweep direction of a step's launches -- which orders the additions of its kinetic-energy sums -- is fixed from
 * the step counter when the step is ENQUEUED (step k starts in direction k & 1, see "What is reproducible bit for bit" above), so a recording bakes
 * its directions in.  A graph of an EVEN number of steps replays the eager loop's launches exactly; a graph of an odd number
 * does so on every other replay only -- record two graphs back to back and replay them in turn (HipContext.capture_steps does)
 * if the trajectory is to be the eager one bit for bit.  Either way the result is correct to rounding. */
tgnh_status tgnh_note_replayed_steps(tgnh_handle h, int nsteps);
/* What the handle still owes the trajectory, as a bit set (inspection only; a caller that records steps into a hipGraph
 * checks that the set is the same before and after the recorded steps -- a graph replays launches, not decisions):
 * bit 0 the end half of the last step waits for the next tgnh_step_begin (RESIDENT_STEP), 1 velm lags by the scale factors,
 * 2 velm lags by the second half kick, 3 the next step's first thermostat half has already run (DEFER_SCALE), 4 the summed
 * kinetic energies wait for the next rescale launch to run the chain, 5 the partial rows are not summed yet, 6 an exchange is
 * sent but not yet waited for, 7 the advanced thermostat block sits in the staging copy, 8 direction of the next sweep,
 * 9 the next thermostat half step starts from the kinetic energies the last one left (TGNH_FLAG_TRUST_STATE_CHANGED),
 * 10 the velocities live in the library's own x | y | z planes and velm's x, y, z are as old as the last flush or query that
 * needed them (the one-launch step of DEFER_SCALE | RESIDENT_STEP, see tgnh_get_velocity_planes; tgnh_flush brings velm up to date). */
tgnh_status tgnh_get_pending_state(tgnh_handle h, uint32_t* bits);
/* The one-launch step's private velocity layout (inspection only).  A handle whose whole deferred step is one launch over wave
 * tiles of identical molecules keeps the velocities, between two flushes, in three planes of its own without velm's 1/m word:
 * the launch then moves 24 B per slot less (mixed and double precision; a single-precision handle stays on velm).  Results are bit for bit those of a handle that stays on
 * velm; the flush contract is unchanged (tgnh_flush, or any call that hands velocities out, first writes velm).  The planes are
 * entered after out[3] one-launch steps in a row and left by whatever settles velm.  TGNH_VELOCITY_PLANES=0 in the environment
 * at tgnh_create keeps a handle on velm.
 * out[0] 1: the velocities live in the planes now (bit 10 of tgnh_get_pending_state); out[1] 1: this handle can take them (its
 * topology qualifies, they were allocated at create, velm's w has not been found to differ from 1 / mass, and no steps were
 * recorded into a graph while velm held the velocities); out[2] one-launch steps in a row since the last settle; out[3] the
 * threshold. */
tgnh_status tgnh_get_velocity_planes(tgnh_handle h, int32_t out[4]);
/* Restore the clock of a checkpointed run (time, stepCount: ReferenceDrudeTGNHKernels.cpp:413-414, CudaDrudeTGNHKernels.cpp:405-406). */
tgnh_status tgnh_set_time(tgnh_handle h, double time, int64_t step_count);
/* Velocities were changed behind the integrator's back (setVelocities, CMMotionRemover,
 * barostat): cached kinetic energies are stale.  DrudeTGNHIntegrator.cpp:166-170
 * Host-side bookkeeping, with one exception.  While bit 10 of tgnh_get_pending_state is set (a DEFER_SCALE | RESIDENT_STEP
 * handle between tgnh_step_begin and tgnh_step_end: the velocities live in the library's planes) the call first WRITES velm's
 * x, y, z from the planes -- one launch on the stream of the last tgnh_step_begin, which must still exist -- so that the
 * planes are not carried on past the change.  A caller that writes velm on such a handle therefore calls tgnh_flush(stream)
 * first, then writes, then calls this (after the flush bit 10 is clear and nothing is launched here); called after a write that no
 * flush preceded, it overwrites that write.  tgnh_bind_buffers with another velm array does the same for the array that goes.
 * HipContext.setVelocities and the library's own velocity setters keep this order. */
tgnh_status tgnh_state_changed(tgnh_handle h);

/* Context::setVelocitiesToTemperature for a Drude system: draws x, y, z of EVERY slot of the bound velm on the device, one
 * launch on `stream`; w stays bit for bit what it is, positions, forces and the thermostat are not touched.  A per-particle
 * Maxwell-Boltzmann draw would put `temperature` into the Drude springs; here a pair's centre of mass is drawn at
 * `temperature` and its relative (Drude) motion at `drude_temperature`.  Per slot, with m = 1 / w (as every step kernel reads
 * masses), kB the descriptor's and z(i) three standard normals of global index i:
 *   massless slot (w == 0)   v = 0
 *   slot in no pair          v = sqrt(kB T / m) z(own index)
 *   pair, Drude d, parent p  mt = m_d + m_p, mu = m_d m_p / mt,
 *                            v_cm = sqrt(kB T / mt) z(p),  v_rel = sqrt(kB T_D / mu) z(d)      (v_rel = v_p - v_d)
 *                            v_d = v_cm - v_rel (m_p / mt),  v_p = v_cm + v_rel (m_d / mt)
 * Random numbers: z(i) depends on (seed, global index) alone, global index = first_particle + the slot's index in this handle
 * (a shard passes the index of its first slot in the whole system).  Philox4x32-10 with key = (low word of seed, high word of
 * seed) and counter = (low word of the global index, high word, 0, 0); its four output words x0..x3 become uniforms
 * u_k = (x_k + 0.5) 2^-32 in fp64, and
 *   z = ( r0 cos(2 pi u1), r0 sin(2 pi u1), r1 cos(2 pi u3) ),  r0 = sqrt(-2 ln u0),  r1 = sqrt(-2 ln u2)
 * (the fourth normal is discarded).  Everything is computed in fp64 and stored in velm's type.  No state is kept between calls
 * and nothing depends on tiling, step path, grid, device or sharding: a particle gets the same velocity wherever and however
 * it is generated.  dualNH and TGNH handles draw alike (temperature groups play no part).
 * NOT done, as in OpenMM: no removal of the total momentum (tgnh_remove_cm_motion afterwards does that), no rescale to the exact target (tgnh_rescale_to_temperature afterwards does that), no constraint projection (under
 * constraints run the velocity-constraint call-out afterwards).
 * The call is a setVelocities: before anything is written it does what tgnh_state_changed does -- refused with that call's
 * status between the steps of a TGNH_FLAG_DEFER_SCALE sequence (velm untouched); afterwards bit 9 of tgnh_get_pending_state is
 * clear and a cached kinetic-energy sum is stale (ke_sum_valid = 0).
 * TGNH_ERR_ARG: a temperature that is negative or not finite (0 is legal: exact zeros), first_particle < 0.  TGNH_ERR_STATE:
 * buffers not bound, a host-only handle. */
tgnh_status tgnh_set_velocities_to_temperature(tgnh_handle h, double temperature, double drude_temperature,
                                               uint64_t seed, int64_t first_particle, void* stream);

/* Centre-of-mass motion: the total mass and momentum of the bound velocities, and their removal (OpenMM's CMMotionRemover).
 * tgnh_desc.has_cm_motion_remover only takes the three degrees of freedom off the thermostats; these calls do the removing -- for
 * a host without OpenMM, for a particle-sharded run (no component outside the library sees every rank's momentum), and after
 * tgnh_set_velocities_to_temperature, which leaves a net momentum of order sqrt(N) thermal momenta in the box.
 * Per slot of the bound velm, everything in fp64, each product and each sum rounded on its own (no fused multiply-add):
 *   massive slot (w != 0)    m = 1.0 / (double)w;   the slot adds m to M and m (double)vx, m (double)vy, m (double)vz to P
 *   massless slot (w == 0)   adds nothing, is not counted in `massive`, and is never written
 *   v_cm = P / M (three IEEE divisions);   removal / shift:  v' = (type of velm)((double)v - d), d = v_cm or dv, rounded once;
 *   w is stored back bit for bit.  M == 0 (no massive slot): nothing is written.
 * Reproducible as the header's rules above have it: no floating-point atomic; the grid of the summing pass is a function of
 * num_particles alone (ceil(N / 256) work-groups, at most 1024, a grid-stride loop beyond) and every order of additions is fixed by
 * it -- a thread adds its slots in ascending index order, a wavefront its lanes, a work-group its wavefronts and one work-group the
 * rows, each in a fixed order -- so the same velm gives the same bits from any handle over the same slots: tiled or TGNH_FLAG_GATHER,
 * dualNH or TGNH, whatever the flags, asked once or twice.  Every thread of the shift divides the same P by the same M.
 *
 * tgnh_get_momentum: a query.  Like tgnh_get_kinetic_energy it first applies what a step has left owed to velm (tgnh_flush); it
 * changes nothing else of the trajectory and leaves the sweep direction as it found it.  It synchronises `stream` and follows
 * tgnh_get_status_flags' rule for sticky failures.  SHARDED RUNS: the answer is for THIS handle's slots; mass, momentum and massive
 * are additive over ranks.  TGNH_ERR_ARG: out is NULL or out->struct_size is not sizeof(tgnh_momentum) (set it before the call;
 * nothing else of *out is read, and on an error nothing of it is written).  TGNH_ERR_STATE: buffers not bound, a host-only handle.
 *
 * tgnh_remove_cm_motion: v' = v - v_cm for every massive slot.  A setVelocities: before anything is written it does what
 * tgnh_state_changed does -- refused with that call's status where that call is refused (between the steps of a
 * TGNH_FLAG_DEFER_SCALE sequence; velm untouched) -- and afterwards bit 9 of tgnh_get_pending_state is clear and a cached
 * kinetic-energy sum is stale (ke_sum_valid = 0).  It enqueues, on `stream` and without waiting for the device: the summing pass,
 * the sum of its rows, then -- SHARDED RUNS -- the four doubles {M, Px, Py, Pz} through the all-reduce of tgnh_set_allreduce or the
 * library's own RCCL (count 4, in place, the same call that carries the kinetic-energy sums; collective: every rank calls this
 * between the same two steps), and the shift.  Every rank then divides the same sums: the same v_cm bits everywhere.  Capturable
 * into a hipGraph like every launch of a step (the first call on a handle allocates a few KiB of scratch: make it, or
 * tgnh_set_cm_motion_removal, outside the capture).  With a MAILBOX exchange attached: TGNH_ERR_UNSUPPORTED -- the mailboxes carry
 * the kinetic-energy sums only; such a caller takes tgnh_get_momentum on every rank, adds the sums by its own means and calls
 * tgnh_shift_velocities with the same dv on every rank.  TGNH_ERR_STATE: buffers not bound, a host-only handle.
 *
 * tgnh_shift_velocities: v' = v - dv for every massive slot, one launch.  Refuses and invalidates as tgnh_remove_cm_motion does (a
 * mailbox exchange does not refuse it).  TGNH_ERR_ARG: dv is NULL or a component is not finite.  dv is read before the call returns.
 *
 * tgnh_set_cm_motion_removal(every): a CMMotionRemover inside the step loops.  every = 0 (the default): off.  every > 0:
 * tgnh_step_begin and tgnh_step_begin_kick look at the step count (tgnh_get_time) BEFORE the step; if it is a multiple of `every`
 * they enqueue tgnh_remove_cm_motion's launches before their own first launch and drop the kinetic energies carried under
 * TGNH_FLAG_TRUST_STATE_CHANGED.  So tgnh_run_harness, tgnh_run_harness_constrained, tgnh_run_steps and any loop over the step
 * entry points remove the drift every `every` steps.  (This is believed to be the step at which OpenMM's CMMotionRemover acts --
 * in updateContextState, ahead of the integrator's step, when the step count is a multiple of its frequency; OpenMM was not at
 * hand to check against.)  Inside OpenMM leave it off: the System's own CMMotionRemover keeps acting there.  SHARDED RUNS: every
 * rank sets the same value.  A hipGraph of steps bakes in the removals of the steps it recorded: record a multiple of `every`
 * steps, from a step count that is one.  TGNH_ERR_ARG: every < 0.  TGNH_ERR_UNSUPPORTED: every > 0 on a handle that steps with
 * TGNH_FLAG_DEFER_SCALE (its velocities lag between steps) or has a mailbox exchange attached; and tgnh_exchange_attach /
 * _attach_pointers return it while removal is on. */
typedef struct tgnh_momentum {
    uint32_t struct_size;     /* in: sizeof(tgnh_momentum); anything else: TGNH_ERR_ARG */
    int32_t  reserved;        /* out: 0 */
    int64_t  massive;         /* slots with w != 0 */
    double   mass;            /* M */
    double   momentum[3];     /* P */
} tgnh_momentum;
tgnh_status tgnh_get_momentum(tgnh_handle h, void* stream, tgnh_momentum* out);
tgnh_status tgnh_shift_velocities(tgnh_handle h, const double dv[3], void* stream);
tgnh_status tgnh_remove_cm_motion(tgnh_handle h, void* stream);
tgnh_status tgnh_set_cm_motion_removal(tgnh_handle h, int every);

/* Scaling the molecules' centres: the coordinate move of a Monte Carlo barostat (OpenMM's MonteCarloBarostat rescales the box and
 * the molecule centres; the reference's example runs one, example/nacl_tg.py:13-14, 56-57) for a host without OpenMM and for a
 * particle-sharded run, without the positions leaving the device.  A barostat must move each molecule RIGIDLY: scaled per particle,
 * every Drude-parent distance and every constrained bond would be scaled too, and the hard wall would be hit by the barostat
 * instead of by the physics.  So these calls know molecules.
 *
 * THE MOLECULE TABLE.  tgnh_set_molecules: molecule[i] is any int32 label; slots with equal labels form one molecule, whether or
 * not they are consecutive.  NULL selects the default: the descriptor's resid where the handle was given one, in either mode --
 * here a residue stored in several runs is ONE molecule, unlike the reference's centre-of-mass walk (see
 * tgnh_rescale_to_temperature's limit).  Without resid (DUALNH created with resid = NULL) there is no default: TGNH_ERR_STATE,
 * "call tgnh_set_molecules first", from every call that needs a table, until labels are set.  A handle that never calls
 * tgnh_set_molecules has the default table, resolved at the first call that needs one.  tgnh_get_molecules returns the labels
 * renumbered in order of first appearance, 0..M-1; tgnh_get_num_molecules returns M (a barostat's acceptance rule needs it).  All
 * three work on a host-only handle.  TGNH_ERR_ARG: a Drude pair whose two members carry different labels -- the move would
 * stretch the spring; the message names the pair.  The default table gets the same check, so a resid that splits a pair fails
 * with that message.  A refused table leaves the one in force as it was.  Constraints are NOT checked: the handle does not keep
 * them (tgnh_desc.constraint_i / _j are read by tgnh_create only); the caller sees to it that no constraint crosses a molecule.
 * SHARDED RUNS: shards are whole molecules already; nothing is exchanged, and every rank passes the same scale.
 *
 * tgnh_scale_positions.  Everything in fp64, every operation rounded on its own (no fused multiply-add).  Per component, with
 * x(i) the coordinate as tgnh_get_drude_statistics defines it (posq, plus posq_correction in mixed precision):
 *   S  = the sum of x(i) over the molecule's n members, massless slots included (virtual sites move with their molecule)
 *        n <= 64: in ascending slot order, left to right, starting from the first member's value
 *        n  > 64: in an order that is a function of the member list alone (not of the grid, the device, the flags or the step
 *                 path): lane l of one wavefront adds members l, l + 64, ... in ascending order onto 0.0, then the 64 lanes are added
 *   c  = S / (double)n                     one IEEE division
 *   d  = c * (scale - 1.0)                 (scale - 1.0) formed once, on the host
 *   x' = x(i) + d
 *   stored:  double  posq = x'
 *            single  posq = (float)x'
 *            mixed   posq = hi = (float)x',  posq_correction = (float)(x' - (double)hi)
 * posq.w (the charge) and posq_correction.w are stored back bit for bit.  NO periodic box is known and nothing is wrapped:
 * molecules scale about the origin, and the caller scales its own box vectors.  OpenMM scales about the box's centre and wraps
 * molecules back into the box; the two differ only by whole box vectors.  The same positions give the same bits from any handle
 * over the same slots and the same molecule table: tiled or TGNH_FLAG_GATHER, TGNH or DUALNH, whatever the flags, asked once or
 * twice from the same positions.  scale = (1, 1, 1) leaves every value bit for bit in double and single precision (d = +-0); in
 * mixed precision the hi / lo split is re-normalised: hi + lo is unchanged, the two parts need not be.
 * It enqueues on `stream`; nothing waits for the device; capturable into a hipGraph.  The device copies of the molecule table (and
 * the table path's 24 bytes per molecule of scratch) are made at tgnh_set_molecules on a device handle or at the first launching
 * call -- never inside a capture: a first call on a capturing stream returns TGNH_ERR_STATE and says so.  One launch where every
 * molecule is a run of consecutive slots no longer than a wavefront (each slot read once and written once), two launches by
 * global index otherwise (members that are not consecutive, molecules longer than 64 slots).
 * save != 0: the same launch also stores what it read into a snapshot owned by the handle -- a trial move is ONE launch.  The
 * snapshot is one copy of posq, and of posq_correction in mixed precision, allocated at the first such call.
 * Positions are not velocities: the call does NOT do what tgnh_state_changed does.  The kinetic energies carried under
 * TGNH_FLAG_TRUST_STATE_CHANGED, the sweep direction, tgnh_get_pending_state and the thermostat stay as they are.
 * REFUSED while a half kick is still owed to velm -- bit 0 or bit 2 of tgnh_get_pending_state -- with TGNH_ERR_STATE and the
 * positions untouched: that kick belongs to the forces of the old positions, and the folded launch of the next tgnh_step_begin
 * would take it from the forces of the new ones.  THE CALLER'S TWO DUTIES: call tgnh_flush first; and after every successful
 * call recompute the forces into the bound force buffer before the next step (the buffer holds the forces of the old positions).
 * The harness' tether sites (tgnh_harness_pack_sites) are not scaled.
 * TGNH_ERR_ARG, checked first so that a host-only handle answers it: scale is NULL, or a component is not finite or <= 0.
 * TGNH_ERR_STATE: buffers not bound, a host-only handle, no molecule table and no resid.  Follows tgnh_get_status_flags' rule for
 * sticky failures, as the step entry points do.
 *
 * tgnh_restore_positions: copies the snapshot back over posq and posq_correction, on `stream`: bit for bit what the saving call
 * read, w included.  The snapshot stays valid until the next saving call: it can be restored twice.  TGNH_ERR_STATE: no
 * snapshot, or tgnh_bind_buffers has rebound posq or posq_correction since it was taken; buffers not bound, a host-only handle. */
tgnh_status tgnh_set_molecules(tgnh_handle h, const int32_t* molecule /* [N] or NULL */);
tgnh_status tgnh_get_num_molecules(tgnh_handle h, int* count);
tgnh_status tgnh_get_molecules(tgnh_handle h, int32_t* molecule_out /* [N] */);
tgnh_status tgnh_scale_positions(tgnh_handle h, const double scale[3], int save, void* stream);
tgnh_status tgnh_restore_positions(tgnh_handle h, void* stream);

/* Energy minimisation on the device: FIRE (Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201, 2006) between
 * the caller's force call-outs -- what the reference's example takes from OpenMM as simulation.minimizeEnergy (example/nacl_tg.py),
 * for a host without OpenMM and for a particle-sharded run, without the positions leaving the device.  For a Drude system the call
 * is not optional: a model builder puts every Drude particle on its parent, and a run must relax them before its first step.  The
 * library knows no potential energy, so the method needs forces only; its accept / reset decision is three sums and lives on the
 * device: a batch of {force call-out, tgnh_minimize_iterate} is enqueued with no host round trip.
 *
 * tgnh_minimize_begin(desc, work).  WHICH SLOTS MOVE: a slot moves if its mass in the descriptor is non-zero (virtual sites never
 * move: the caller's virtual-site call-out places them), AND desc->moving is NULL or non-zero there, AND -- with
 * TGNH_MIN_DRUDE_ONLY -- it is a Drude slot (pair_drude).  The mask, one byte per slot, is formed on the host and uploaded once.
 * `work` is device memory of the caller's, 3 N doubles, the minimiser's velocity in planes work[k N + i], fp64 in every precision;
 * begin zeroes it and initialises the state block on the device (dt = dt_start, alpha = alpha_start, all counters 0), then waits
 * for `stream`.  A begin on a capturing stream returns TGNH_ERR_STATE and says so.  A begin while a minimisation is under way
 * starts anew.  Units: masses are 1, so a displacement is dt^2 f with f in kJ/mol/nm: dt is not a time.
 *
 * tgnh_minimize_iterate: ONE ITERATION on whatever the bound force buffer holds.  Everything in fp64, every operation rounded on
 * its own (no fused multiply-add).
 *   1. SUMS over the moving slots, with f_k = (double)F_k[i] / 4294967296.0 (F the fixed-point force) and v_k = work[k N + i]:
 *        P  = sum of (fx vx + fy vy) + fz vz        FF = sum of (fx fx + fy fy) + fz fz
 *        VV = sum of (vx vx + vy vy) + vz vz        moving = sum of 1.0
 *      added in exactly tgnh_get_momentum's order: the grid is a function of N alone (256 slots per work-group, at most 1024
 *      work-groups, a grid-stride loop beyond); a thread adds its slots in ascending index order onto 0.0; a wavefront adds its 64
 *      lanes in a fixed order; a work-group its wavefronts in wavefront order; one work-group adds the rows -- thread t the run of
 *      consecutive rows [t c, (t + 1) c), c = ceil(rows / 256), then as a work-group does.  No floating-point atomic: the same
 *      forces, `work` and mask give the same bits from any handle over the same slots.
 *   2. EXCHANGE.  Where the handle has an all-reduce (tgnh_set_allreduce, or the library's RCCL) the four doubles
 *      {P, FF, VV, moving} go through it in place, in one call of count 4.  SHARDED RUNS: the call is collective.
 *   3. DECISION, by one thread on the device, on the state block.  Once converged != 0 the block stays as it is.  Otherwise
 *        rms = sqrt(FF / (3.0 * moving));  the four sums and rms are stored
 *        a sum is not finite:   converged = -1, nothing else changes
 *        rms <= tolerance:      converged = 1, nothing else changes
 *        iterations == 0:       a = 1, b = 0, dt and alpha as they are
 *        P > 0:                 since_uphill++;  a = 1.0 - alpha;  b = (alpha * sqrt(VV)) / sqrt(FF);
 *                               if since_uphill > n_min:  dt = min(dt * f_inc, dt_max);  alpha = alpha * f_alpha
 *        else:                  uphill++;  since_uphill = 0;  a = b = 0;  dt = dt * f_dec;  alpha = alpha_start
 *        then iterations++      (iterations counts updates: the decision that finds convergence does not count)
 *      The mix uses alpha before its update; the update below uses dt after its update.
 *   4. UPDATE, per moving slot and component k, unless converged != 0 (then this and every later update launch returns at once:
 *      the positions stay those at which the converged forces were computed; a run that blew up stays as evidence):
 *        v'  = (a * v) + (b * f);   v'' = v' + dt * f;   d = dt * v'';   r = sqrt((dx dx + dy dy) + dz dz)
 *        r > max_step:  s = max_step / r (one division), every d = d * s
 *        x'  = x + d, x as tgnh_scale_positions reads it and stored as tgnh_scale_positions stores it (mixed precision: hi / lo
 *              re-normalised); posq.w and posq_correction.w go back bit for bit;  work = v'' (not scaled by s)
 *      A slot that does not move is neither loaded nor written.
 * Without an all-reduce the row sum and the decision share a launch (three launches an iteration); with one the decision is a
 * launch of its own behind the hook (four).  The bits are the same.  Nothing waits for the device: capturable into a hipGraph.
 *
 * WHAT THE CALLS ARE NOT.  Like tgnh_scale_positions they are not a tgnh_state_changed: velm, the carried kinetic energies, the
 * sweep direction, tgnh_get_pending_state, the thermostat and tgnh_scale_positions' snapshot stay as they are.  Begin and iterate
 * are REFUSED with TGNH_ERR_STATE, positions untouched, while a half kick is owed to velm (bit 0 or 2 of tgnh_get_pending_state:
 * tgnh_flush first).  The hard wall is not applied; tgnh_get_drude_statistics tells afterwards.  CONSTRAINTS are call-outs the
 * minimiser does not make: a caller with constraints moves only slots no constraint touches (TGNH_MIN_DRUDE_ONLY, or a mask), or
 * projects itself.  The caller recomputes the forces before the next step unless the minimisation ended converged = 1 (then the
 * buffer holds the forces of the positions as they are).
 *
 * tgnh_get_minimize_state: the state block as the last decision left it (`moving`: this handle's own moving slots).  A query:
 * synchronises `stream`.  tgnh_minimize_end frees mask, rows and state block (not `work`: the caller's); harmless without a begin.
 * tgnh_run_harness_minimize: `iterations` x {the harness force into the bound force buffer, tgnh_minimize_iterate}, enqueued back
 * to back, as tgnh_run_harness enqueues steps.
 *
 * TGNH_ERR_ARG, checked first so that a host-only handle answers it: desc or work is NULL, a parameter that is not finite,
 * tolerance < 0, dt_start <= 0, dt_max < dt_start, max_step <= 0, f_inc < 1, f_dec or f_alpha outside (0, 1), alpha_start outside
 * (0, 1], n_min < 0, unknown flag bits; a NULL `out`; iterations < 0.  TGNH_ERR_UNSUPPORTED: a MAILBOX exchange is attached (it
 * carries the kinetic-energy sums only).  TGNH_ERR_STATE: buffers not bound, a host-only handle, iterate / get / run without a
 * begin, no slot moves, a capturing stream at begin, an owed half kick.  Follows tgnh_get_status_flags' rule for sticky failures. */
enum { TGNH_MIN_DRUDE_ONLY = 1 };
typedef struct tgnh_minimize_desc {
    double tolerance;          /* kJ/mol/nm: stop when the root mean square of the moving slots' force components is <= this (OpenMM's rule; its default 10) */
    double dt_start, dt_max;   /* unit masses: a displacement is dt^2 f.  The Python layer's defaults: 1e-4, 1e-3 */
    double max_step;           /* nm, per slot and iteration; default 0.01 */
    double f_inc, f_dec, alpha_start, f_alpha;   /* 1.1, 0.5, 0.1, 0.99 */
    int32_t n_min;             /* 5 */
    int32_t flags;             /* TGNH_MIN_DRUDE_ONLY: only Drude slots move; any other bit: TGNH_ERR_ARG */
    const uint8_t* moving;     /* host, [N] or NULL: a slot moves only where this is non-zero */
} tgnh_minimize_desc;
typedef struct tgnh_minimize_state {
    int64_t iterations, uphill, since_uphill, moving;
    int32_t converged;         /* 0 running, 1 rms <= tolerance, -1 a sum was not finite */
    int32_t reserved;
    double dt, alpha, power, ff, vv, rms_force;   /* of the last decision */
} tgnh_minimize_state;
tgnh_status tgnh_minimize_begin(tgnh_handle h, const tgnh_minimize_desc* desc, double* work /* device, 3 N doubles, the caller's */, void* stream);
tgnh_status tgnh_minimize_iterate(tgnh_handle h, void* stream);
tgnh_status tgnh_get_minimize_state(tgnh_handle h, void* stream, tgnh_minimize_state* out);   /* synchronises */
tgnh_status tgnh_minimize_end(tgnh_handle h);
tgnh_status tgnh_run_harness_minimize(tgnh_handle h, const void* x0, double k_drude, double k_tether, int iterations, void* stream);

/* The periodic box, whole molecules wrapped into it on the device, and compact fp32 frames: what the reference's example takes
 * from OpenMM as getState(getPositions=True, enforcePeriodicBox=True) and DCDReporter (example/nacl_tg.py), for a host without
 * OpenMM and for a particle-sharded run, without the fp64 positions leaving the device.  A run whose barostat scales its molecules
 * (tgnh_scale_positions) and never wraps lets them diffuse out of the cell: coordinates grow, and in single and mixed precision
 * that costs position bits.
 *
 * THE BOX.  tgnh_set_periodic_box takes the three box vectors in OpenMM's reduced form, as Context::setPeriodicBoxVectors demands
 * it (recalled from OpenMM's documentation; OpenMM was not at hand to check against):
 *   a = (ax, 0, 0),  b = (bx, by, 0),  c = (cx, cy, cz);   ax, by, cz > 0;   ax >= 2 |bx|,  ax >= 2 |cx|,  by >= 2 |cy|;
 *   every component finite.
 * Anything else: TGNH_ERR_ARG, and the box in force stays as it was.  The box is kept on the host -- the call works on a host-only
 * handle -- and tgnh_get_periodic_box returns the stored doubles bit for bit (TGNH_ERR_STATE before the first set).  It travels
 * with each launch by value, as tgnh_scale_velocities' factors do: a recorded hipGraph bakes in the box it was recorded with.
 * tgnh_scale_positions does not touch the box: the caller sets the new one after an accepted move.  SHARDED RUNS: every rank sets
 * the same box; nothing is exchanged.
 *
 * tgnh_wrap_molecules.  Per molecule of the table in force (THE MOLECULE TABLE above: the same default, the same TGNH_ERR_STATE
 * without one), everything in fp64, every operation rounded on its own (no fused multiply-add).  S, n and c = S / (double)n are
 * exactly tgnh_scale_positions': the same coordinates x(i), the same order of additions for n <= 64 and for n > 64.  Then
 *   kz = floor(c_z / cz);            d = (kz cx, kz cy, kz cz)
 *   ky = floor((c_y - d_y) / by);    d_x = d_x + ky bx;   d_y = d_y + ky by
 *   kx = floor((c_x - d_x) / ax);    d_x = d_x + kx ax
 * -- OpenMM's enforcePeriodicBox arithmetic as recalled: molecule centres into the cell [0, L), z first.  A molecule with
 * kx == ky == kz == 0, or with a centroid that is not finite, is NOT WRITTEN AT ALL: its posq and posq_correction stay bit for bit
 * (in mixed precision the hi / lo split is not re-normalised; the positions of a run that has blown up stay as evidence).  Every
 * other molecule: x' = x(i) - d, stored exactly as tgnh_scale_positions stores; posq.w and posq_correction.w are stored back bit
 * for bit.  Cell indices are integers and d is formed from them and the box alone: the same positions, table and box give the same
 * bits from any handle -- tiled or TGNH_FLAG_GATHER, TGNH or DUALNH, asked once or twice from the same positions.
 * It enqueues on `stream`, waits for nothing and is capturable; the device tables are made outside a capture by
 * tgnh_scale_positions' rule (a first call on a capturing stream: TGNH_ERR_STATE).  Positions are not velocities: the call does NOT
 * do what tgnh_state_changed does; tgnh_get_pending_state, the carried kinetic energies, the sweep direction and the thermostat
 * stay as they are.  It is NOT refused while a half kick is owed to velm: the forces of a periodic system do not change when a
 * whole molecule moves by box vectors, so the owed kick is the same kick.  The harness' tether force is NOT periodic and its sites
 * are not moved: a caller of tgnh_run_harness* does not wrap.  The snapshot of tgnh_scale_positions(save) is left alone: a
 * tgnh_restore_positions after a wrap gives the positions from before it.
 * TGNH_ERR_STATE: no box set (checked first, so a host-only handle answers it); then: buffers not bound, a host-only handle, no
 * molecule table and no resid.  Follows tgnh_get_status_flags' rule for sticky failures, as the step entry points do.
 *
 * tgnh_write_frame: ONE READ-ONLY pass over the bound positions that leaves fp32 coordinates in `out`, a device pointer of the
 * caller's.  It never writes posq, posq_correction or anything else of the trajectory; it needs no tgnh_flush (only velm ever
 * lags), does not synchronise and is capturable.  Per slot i and output index j, in fp64 and rounded once to float:
 *   value = (float)((x(i) - d) * unit)
 * with d the slot's molecule's shift as above under TGNH_FRAME_WRAP, and d = +0.0 without the flag or for a molecule that
 * tgnh_wrap_molecules would not move.  Planar layout (the default; what a DCD record is): component k at out[k * stride + j];
 * TGNH_FRAME_INTERLEAVED: component k at out[3 j + k].  Floats of `out` that are no coordinate -- the gap between count and stride,
 * anything beyond -- are not written.  j = i; with TGNH_FRAME_SKIP_DRUDE the Drude slots (pair_drude) are left out and j = i minus
 * the number of Drude slots below i.  tgnh_get_frame_count returns the number of output indices, N or N minus the Drude slots, on a
 * host-only handle too.  Without TGNH_FRAME_WRAP the call needs neither a box nor a molecule table: a DUALNH handle created without
 * resid can write frames.  Out of scope: writing straight into pinned host memory; the caller copies the frame.
 * TGNH_ERR_ARG, checked first so that a host-only handle answers it: desc or out is NULL, desc->struct_size is not
 * sizeof(tgnh_frame_desc), an unknown flag, unit not finite or <= 0, stride < count (planar) or stride != 0 (interleaved), capacity
 * smaller than 2 stride + count (planar) or 3 count (interleaved); and where the runtime knows the allocation behind `out`, fewer
 * than `capacity` floats behind the pointer (not looked at on a capturing stream).  TGNH_ERR_STATE: TGNH_FRAME_WRAP without a box or
 * without a molecule table, buffers not bound, a host-only handle; on a capturing stream, a table the call needs that is not on the
 * device yet (call once with the same flags outside the capture).  SHARDED RUNS: every rank writes its own slots. */
tgnh_status tgnh_set_periodic_box(tgnh_handle h, const double a[3], const double b[3], const double c[3]);
tgnh_status tgnh_get_periodic_box(tgnh_handle h, double a[3], double b[3], double c[3]);
tgnh_status tgnh_wrap_molecules(tgnh_handle h, void* stream);
enum { TGNH_FRAME_WRAP = 1, TGNH_FRAME_SKIP_DRUDE = 2, TGNH_FRAME_INTERLEAVED = 4 };
typedef struct tgnh_frame_desc {
    uint32_t struct_size;   /* sizeof(tgnh_frame_desc); anything else: TGNH_ERR_ARG */
    int32_t  flags;         /* TGNH_FRAME_*; any other bit: TGNH_ERR_ARG */
    double   unit;          /* every coordinate is multiplied by it (10.0: nm -> Angstrom, DCD's unit) */
    int64_t  stride;        /* planar layout: floats between the x, y and z planes, >= count; interleaved: must be 0 */
    int64_t  capacity;      /* floats behind `out` */
} tgnh_frame_desc;
tgnh_status tgnh_get_frame_count(tgnh_handle h, int32_t flags, int64_t* count);
tgnh_status tgnh_write_frame(tgnh_handle h, const tgnh_frame_desc* desc, float* out /* device */, void* stream);

/* Velocity rescaling: one factor per thermostat applied to the bound velocities the way the integrator's own rescale applies the
 * chain's (ReferenceDrudeTGNHKernels.cpp:516-541; CUDA kernel integrateDrudeTGNHChain), and the factors that put every thermostat's
 * kinetic energy onto its N kT at once -- an exact-temperature start after tgnh_set_velocities_to_temperature, velocity-rescaling
 * equilibration (a Nose-Hoover chain started far from its target rings for a long time), a replica-exchange swap
 * (factor sqrt(T_new / T_old) per bath), a quench.  With factors s[NT] in tgnh_get_last_scale_factors' layout -- TGNH
 * [groups.., COM, Drude], DUALNH [real, unused, Drude]; the unused entry is not looked at:
 *   TGNH    ordinary slot of group g   v' = s[g] (v - v_com) + s[COM] v_com        v_com: its molecule's centre-of-mass velocity
 *           pair (group of the Drude)  its centre of mass as an ordinary slot, its relative motion v_parent - v_Drude by s[Drude]
 *           (COM group off: v_com = 0 and s[COM] plays no part)
 *   DUALNH  ordinary slot v' = s[real] v;  pair: centre of mass by s[real], relative motion by s[Drude]
 * This is not a second statement of that arithmetic: the launch IS the step's rescale launch (tiled, wave-tile or gather form,
 * whichever the handle steps with), reading its factors from scratch of these calls instead of the thermostat block.  Massless
 * slots and every w stay bit for bit.  The thermostat block is not written: tgnh_get_last_scale_factors keeps answering for the
 * chain; eta, etaDot and the baths (tgnh_get_dof) stay.
 *
 * tgnh_scale_velocities: the caller's factors.  A setVelocities: before anything is written it does what tgnh_state_changed does
 * -- refused with that call's status where that call is refused (between the steps of a TGNH_FLAG_DEFER_SCALE sequence; velm
 * untouched) -- and afterwards bit 9 of tgnh_get_pending_state is clear and a cached kinetic-energy sum is stale
 * (ke_sum_valid = 0).  The sweep direction (bit 8) is left as it was found: a run that never calls this keeps its bits, one that
 * does is reproducible.  One streaming launch on `stream` (molecules longer than a tile: their centre-of-mass table is computed
 * before it and again after it), nothing waits for the device.  `factors` is read before the call returns -- the values travel
 * with a launch, by value: calls enqueued back to back each apply their own, and the caller's array is free at once.  Capturable
 * into a hipGraph (the first call on a handle allocates 16 NT bytes of scratch: make it, or tgnh_set_velocity_rescaling, outside
 * the capture).  SHARDED RUNS: every rank passes the same factors.  TGNH_ERR_ARG (checked first, so a host-only handle answers
 * them): factors is NULL, count is not NT (tgnh_get_num_thermostats), a factor is negative or not finite (0 is legal: exact
 * zeros).  TGNH_ERR_STATE: buffers not bound, a host-only handle.
 *
 * tgnh_rescale_to_temperature: on `stream`, with no host synchronisation in between: the kinetic-energy pass of the velocities
 * as they are and the sum of its rows (tgnh_compute_kinetic_energies' launches, in the step's own order of additions: a chain
 * still owed or a staged thermostat block is settled first), the handle's all-reduce where one is set (tgnh_set_allreduce or
 * the library's RCCL: the same NT-value call the step makes -- SHARDED RUNS: the call is collective, every rank makes it
 * between the same two steps with the same temperatures), one small kernel that turns sums into factors, and the rescale with them.
 * Per thermostat k, in fp64, every operation rounded on its own:
 *   target_k = the N kT tgnh_get_dof would report if the baths stood at (temperature, drude_temperature): formed on the host by
 *              the functions tgnh_create and tgnh_set_temperatures use, from the handle's (global) degrees of freedom; the
 *              handle's baths are not touched
 *   inert thermostat (no degrees of freedom: N kT = 0 at any temperature -- the COM group switched off, DUALNH's unused
 *              entry, a group without degrees of freedom, the Drude bath of a system without pairs)     s_k = 1
 *   KE_k is NaN                           s_k = 1, and status bit 4 is set (as by a chain handed a NaN sum)
 *   KE_k > 0                              s_k = sqrt(target_k / KE_k): one division, one square root (0 when the temperature is 0)
 *   KE_k == 0                             s_k = 1
 * KE_k, the sums before scaling (no 1/2), are what tgnh_get_last_kinetic_energies returns afterwards.  Refuses and invalidates as
 * tgnh_scale_velocities does.  The factors of two handles over the same velocities agree as their kinetic-energy sums do (1e-12
 * relative between different orders of additions); the same handle asked twice from the same velocities gives the same bits.
 * A LIMIT: where a molecule spans two temperature groups, unequal factors inside it move its centre of mass, and one call does
 * not land on the targets -- a box of 27 SWM4 waters with every hydrogen in a second group misses by 12 %.  The call does not
 * iterate.  (TGNH_FLAG_TRUST_STATE_CHANGED is ignored for such a topology too.)  The same holds where the reference's
 * centre-of-mass walk does not find a molecule's centre of mass: residues stored in several runs with the COM group on (the
 * walk takes `count` consecutive particles from a residue's last run; library and oracle follow it).
 * TGNH_ERR_ARG: a temperature that is negative or not finite.  TGNH_ERR_UNSUPPORTED: a MAILBOX exchange is attached (it carries
 * the step's own sums); such a caller asks tgnh_compute_kinetic_energies on every rank, forms the factors and calls
 * tgnh_scale_velocities alike everywhere.  TGNH_ERR_STATE: buffers not bound, a host-only handle.
 *
 * tgnh_get_rescale_factors: the NT factors the last of the two calls above applied (from tgnh_set_velocity_rescaling's too).  A
 * query: synchronises `stream`, follows tgnh_get_status_flags' rule for sticky failures.  TGNH_ERR_STATE: before the first such
 * call, buffers not bound, a host-only handle.
 *
 * tgnh_set_velocity_rescaling(every, temperature, drude_temperature): the same operation inside the step loops, placed as
 * tgnh_set_cm_motion_removal places the remover.  every = 0 (the default): off.  every > 0: tgnh_step_begin and
 * tgnh_step_begin_kick look at the step count BEFORE the step; if it is a multiple of `every` they enqueue
 * tgnh_rescale_to_temperature's launches before their own first launch -- after a centre-of-mass removal due at the same step --
 * and drop the kinetic energies carried under TGNH_FLAG_TRUST_STATE_CHANGED.  (The step's first thermostat half then runs its own
 * kinetic-energy pass over the scaled velocities; the scaled sums are not handed on.)  SHARDED RUNS: every rank sets the same
 * values.  A hipGraph of steps bakes in the rescalings of the steps it recorded: record a multiple of `every` steps, from a step
 * count that is one.  TGNH_ERR_ARG: every < 0, a temperature that is negative or not finite.  TGNH_ERR_UNSUPPORTED: every > 0 on a
 * handle that steps with TGNH_FLAG_DEFER_SCALE (its velocities lag between steps) or has a mailbox exchange attached; and
 * tgnh_exchange_attach / _attach_pointers return it while rescaling is on. */
tgnh_status tgnh_scale_velocities(tgnh_handle h, const double* factors, int count, void* stream);
tgnh_status tgnh_rescale_to_temperature(tgnh_handle h, double temperature, double drude_temperature, void* stream);
tgnh_status tgnh_get_rescale_factors(tgnh_handle h, void* stream, double* factors);      /* NT doubles; synchronises */
tgnh_status tgnh_set_velocity_rescaling(tgnh_handle h, int every, double temperature, double drude_temperature);

/* Retargets both baths of a live handle (heating, annealing, equilibration at one temperature and production at another):
 * kB T and kB T_D -- the chain's launch arguments and the hard wall's thermal speed --, every N kT and every thermostat mass,
 * all recomputed by the functions tgnh_create runs: bit for bit what a handle created at the new temperatures holds, uploaded
 * on `stream`.  eta, etaDot and etaDotDot stay: the chains run on with their momenta, as a restored checkpoint's would.
 * tgnh_get_dof reports the new N kT.  Refused where tgnh_state_changed is (between the steps of a TGNH_FLAG_DEFER_SCALE sequence
 * a thermostat half has already run at the old temperature); invalidates what tgnh_set_thermostat_state invalidates.
 * TGNH_ERR_ARG: a temperature that is negative or not finite.
 * SHARDED RUNS: the chains are replicated -- every rank must call this with the same values between the same two steps.
 * A hipGraph of steps recorded earlier holds the old kT in its launch arguments: record it again. */
tgnh_status tgnh_set_temperatures(tgnh_handle h, double temperature, double drude_temperature, void* stream);

/* Host-visible results (synchronise `stream`).
 * tgnh_get_kinetic_energy: TGNH mode = the cached 1/2 sum of the last thermostat half step's bins when ke_sum_valid,
 * else 1/2 sum m v^2 (CudaDrudeTGNHKernels.cpp:654-658).  DUALNH mode = 1/2 sum m (v + F dt/2m)^2, the Reference
 * platform's half-step-shifted energy (ReferenceDrudeTGNHKernels.cpp:70-98) WITHOUT its constraint projection, which is
 * a call-out to the host's constraint solver: with constraints present project the shifted velocities first
 * (tests/test_reference_water_gpu.py::reference_platform_kinetic_energy shows the sequence). */
tgnh_status tgnh_get_kinetic_energy(tgnh_handle h, int ke_sum_valid, void* stream, double* out);
tgnh_status tgnh_get_num_thermostats(tgnh_handle h, int* count);               /* NT: TGNH G+2 = [groups.., COM, Drude]; DUALNH 3 = [real, unused, Drude] */
tgnh_status tgnh_get_last_kinetic_energies(tgnh_handle h, void* stream, double* ke);   /* no 1/2; before the chain */
tgnh_status tgnh_get_last_scale_factors(tgnh_handle h, void* stream, double* scale);
/* bit0: a Drude beyond 2x the hard wall; bit1: the harness SHAKE did not converge, or the direct solver's result is outside the tolerance; bit2: a mailbox exchange timed out;
 * bit3: the work-groups of a resident step did not all meet; bit4: a kinetic-energy pass that sums its own rows (tail sum) did not
 * receive every row -- the sums were left as NaN -- or a chain was handed a NaN sum (with an all-reduce attached the NaN of one
 * rank's failed pass reaches every rank, and every rank sets the bit itself).  *flags is always filled in.  bit2, bit3, bit4 -- and bit0 in DUALNH mode, where the Reference platform throws
 * (ReferenceDrudeTGNHKernels.cpp:311-312) -- are FAILURES and sticky: once the host has seen one (here, at any other
 * tgnh_get_*, at tgnh_exchange_detach, or through the read-back the library enqueues behind every 64th step) every later
 * tgnh_step_*, tgnh_flush and tgnh_get_* returns TGNH_ERR_STATE / TGNH_ERR_HARDWALL with the message in tgnh_last_error(). */
tgnh_status tgnh_get_status_flags(tgnh_handle h, void* stream, uint32_t* flags);
tgnh_status tgnh_get_time(tgnh_handle h, double* time, int64_t* step_count);
tgnh_status tgnh_get_dof(tgnh_handle h, double* dof, double* nkt);

/* How the Drude oscillators are doing, from the bound positions as they are: one read-only pass on `stream` over posq (and
 * posq_correction) plus a one-work-group sum, then one small copy to the host.  Per pair (Drude d, parent p), everything in fp64:
 *   coordinate   x(i) = (double)posq[i].x                                   single and double precision
 *                x(i) = (double)posq[i].x + (double)posq_correction[i].x    mixed precision (likewise y, z)
 *   dx = x(d) - x(p), dy, dz likewise;   d2 = dx dx + dy dy + dz dz   (each product and each sum rounded on its own, left to
 *   right: no fused multiply-add);   d = sqrt(d2);   q_D = (double)posq[d].w
 * NO minimum image is applied: the library knows no periodic box, and OpenMM keeps the atoms of a molecule -- a Drude particle and
 * its parent among them -- in one periodic image.  The fields of *out:
 *   pairs           pairs looked at (= num_pairs)
 *   over            pairs with d2 > threshold * threshold
 *   max_distance    sqrt of the largest d2; 0 when there is no pair
 *   worst_particle  slot index, local to this handle, of the Drude particle of the pair with the largest d2 (ties: the lowest
 *                   slot index); -1 when there is no pair
 *   sum_d2          sum of d2 over the pairs (the caller forms rms = sqrt(sum_d2 / pairs))
 *   dipole[3]       sum of q_D dx, q_D dy, q_D dz over the pairs: the induced dipole.  Only the Drude particles' charges enter.
 *   hist            with t = (d * TGNH_DRUDE_HIST_BINS) / hist_max (in fp64): hist[k], k < BINS, counts the pairs with
 *                   floor(t) == k, hist[BINS] those with t >= BINS (that is d >= hist_max).  hist_max == 0 switches the histogram
 *                   off: all entries 0.
 * A query: it reads positions only, so it needs no tgnh_flush (only velm ever lags) and changes nothing of the trajectory nor of
 * tgnh_get_pending_state.  It synchronises `stream`, as every tgnh_get_* does, and follows tgnh_get_status_flags' rule for sticky
 * failures.  Its scratch (a few hundred KiB) is allocated at the first call: a handle that never asks allocates nothing.
 * Reproducible as the header's rules above have it: no floating-point atomic; the grid is a function of num_particles alone (not of
 * the device, the flags or the step path) and every order of additions is fixed by it, so the same positions give the same bits
 * from any handle over the same slots, tiled or TGNH_FLAG_GATHER, asked once or twice.
 * SHARDED RUNS: the library does no exchange for this call; every rank answers for its own slots.  pairs, over, hist, sum_d2 and
 * dipole are additive over ranks (the doubles then to rounding, not to the bits of an unsharded handle), max_distance is a maximum
 * over ranks, worst_particle is local: the caller adds the index of the rank's first slot.
 * TGNH_ERR_ARG: out is NULL, out->struct_size is not sizeof(tgnh_drude_stats) (set it before the call; nothing else of *out is
 * read, and on an error nothing of it is written), threshold or hist_max negative or not finite.  TGNH_ERR_STATE: buffers not
 * bound, a host-only handle.  A handle with num_pairs == 0: TGNH_OK, zeros, worst_particle -1. */
#define TGNH_DRUDE_HIST_BINS 32
typedef struct tgnh_drude_stats {
    uint32_t struct_size;     /* in: sizeof(tgnh_drude_stats); anything else: TGNH_ERR_ARG */
    int32_t  worst_particle;
    int64_t  pairs;
    int64_t  over;
    double   max_distance;
    double   sum_d2;
    double   dipole[3];
    int64_t  hist[TGNH_DRUDE_HIST_BINS + 1];
} tgnh_drude_stats;
tgnh_status tgnh_get_drude_statistics(tgnh_handle h, double threshold, double hist_max, void* stream, tgnh_drude_stats* out);

/* Thermostat state (checkpoint/resume, absent in the reference: SURVEY.md 5).
 * which: 0 eta, 1 etaDot, 2 etaDotDot, 3 etaMass.  Layout: DUALNH = the
 * reference's interleaved vectors; TGNH = [thermostat][link], etaDot rows of C+1. */
tgnh_status tgnh_get_thermostat_len(tgnh_handle h, int which, int* len);
tgnh_status tgnh_get_thermostat_state(tgnh_handle h, int which, void* stream, double* out);
tgnh_status tgnh_set_thermostat_state(tgnh_handle h, int which, void* stream, const double* in);

/* Topology the kernels were built from, for bit-exact index parity (A1).
 * which: 0 normalParticles, 1 pair drude, 2 pair parent, 3 particleTempGroup,
 * 4 particleResId, 5 particlesInResidues.count, 6 particlesInResidues.first,
 * 7 tile starts (num_tiles+1), 8 packed per-slot meta words, 9 wave tiles as (first slot, largest molecule) pairs
 * (one more than tiles; none: a molecule or pair longer than a wavefront), 10 the wave tiles' per-slot words,
 * 11 per 512-slot tile: period | molecules per period << 8 | pattern << 16, 12 per wave tile: period | pattern << 8, where
 * the tile repeats one kind of molecule (or a few) and its kernels form the per-slot words from a pattern instead of
 * reading them (0: they read them), 13 / 14 the patterns of the two, 64 words each, 15 the descriptor masses behind the
 * wave patterns' words, 64 doubles per pattern in 14's order, each as two int32 (a wave pattern is interned by words AND
 * masses; empty where 14 holds its one placeholder row), 16 one word: 1 where every wave tile is patterned and every slot's
 * mass is its pattern entry's bit for bit -- the host's half of what qualifies a handle for the velocity planes --, else 0,
 * 17 where the velocity planes keep a slot (they hold the massive slots only): the stride of a plane in words, the number
 * of bases B (wave tiles + 1), the B bases -- the first word of each wave tile's segment, a multiple of 16, the last one the
 * stride again --, then 64 offsets per wave pattern in 14's order, by lane: the massive slots of the tile before that lane;
 * a massive slot's word is base[tile] + offset[pattern][lane].  0, 0 and nothing else where 16 answers 0.
 * All read-only, all answered by a host-only handle. */
tgnh_status tgnh_get_topology_len(tgnh_handle h, int which, int* len);
tgnh_status tgnh_get_topology(tgnh_handle h, int which, int32_t* out);
/* The sizes the launches of this handle are bound by, against the sizes of what the library allocated for them (inspection;
 * also answered by a host-only handle, for the largest grid any device could give it).  The library checks the same figures
 * before every launch (TGNH_ERR_STATE "internal: ..." instead of a launch that would run off a buffer).  out[8]:
 *   0 512-slot tiles, 1 wave tiles, 2 entries of the wave-tile table (wave tiles + 1; 0: none), 3 the largest grid a streaming
 *   launch of this handle takes, 4 partial rows allocated for such launches, 5 words allocated for tagged rows (0: none),
 *   6 words a launch of grid [3] with this handle's thermostats may write there (0: it never does), 7 thermostats NT. */
tgnh_status tgnh_get_launch_bounds(tgnh_handle h, int32_t out[8]);

/* Pieces of the step, exposed for parity tests of the single kernels. */
tgnh_status tgnh_compute_kinetic_energies(tgnh_handle h, void* stream);          /* A3/A4 only -> last_kinetic_energies */
tgnh_status tgnh_half_kick(tgnh_handle h, void* stream);                         /* A7 only */

/* Harness force (bench/test workload, not part of the reference): Drude spring
 * + tether to sites x0 (real4 [N] device array: x,y,z and w = 1 for a tethered slot, 0 otherwise),
 * written in OpenMM's fixed-point layout into `force_out` (int64 [3*padded]). */
tgnh_status tgnh_harness_force(tgnh_handle h, const void* x0, double k_drude, double k_tether,
                               void* force_out, void* stream);
/* Packs the sites once (synchronous; x0 as above, its writes complete): the tethered slots' sites only, 12 or 24 B each,
 * and one byte per slot in place of the meta word.  Afterwards tgnh_harness_force / tgnh_run_harness* accept x0 = NULL
 * and read the packed form (the same forces bit for bit). */
tgnh_status tgnh_harness_pack_sites(tgnh_handle h, const void* x0);
/* A hint for the next tgnh_harness_pack_sites: the box repeats one molecule of `mol_slots` slots (<= 64) on a simple cubic lattice --
 * this handle's molecule j is molecule m = first_molecule + j of the box (a shard starts in the middle of it), at
 * (m / side^2, (m / side) mod side, m mod side) x spacing, slot k of it at that point + geom[k] (doubles [mol_slots][3]),
 * rounded once to the position type -- as the synthetic water boxes are built.  pack_sites CHECKS every tethered site against that
 * formula, bit for bit, and every slot's role / partner / tether flag against molecule 0's; if all hold, the force kernel forms
 * sites and flags from the slot index and reads nothing but positions (56 B per slot in mixed precision: what it must read and
 * write anyway; 65 B with packed sites); if not, the hint is dropped and the sites are packed as before.  mol_slots = 0 clears it. */
tgnh_status tgnh_harness_lattice_hint(tgnh_handle h, int mol_slots, int side, double spacing, const double* geom, int first_molecule);
/* 0 explicit x0 / nothing packed yet, 1 packed sites, 2 lattice sites (what the last tgnh_harness_pack_sites ended in). */
tgnh_status tgnh_harness_sites_kind(tgnh_handle h, int* kind);
/* nsteps x { step_begin, harness force into the bound force buffer, step_end }
 * enqueued back to back with no host synchronisation. */
/* The step loop with NO call-out: nsteps x (tgnh_step_begin, tgnh_step_end) on whatever the bound force buffer holds.  For
 * timing the integrator's own launches between two synchronisations (bench.py's integrator_only leg zeroes the buffer first:
 * a frozen spring force would drive every Drude particle through its hard wall within ten steps).  Not an integrator of anything. */
tgnh_status tgnh_run_steps(tgnh_handle h, int nsteps, void* stream);
tgnh_status tgnh_run_harness(tgnh_handle h, const void* x0, double k_drude, double k_tether,
                             int nsteps, void* stream);

/* Harness call-outs of the constrained (split) path -- stand-ins for OpenMM's applyConstraints /
 * applyVelocityConstraints / computeVirtualSites (CudaDrudeTGNHKernels.cpp:363, :391, :377), not part of the reference.
 * Clusters: [n][4] slot indices (-1 = unused) and [n][6] distances for the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
 * of a cluster, 0 = unconstrained.  Virtual sites: [n][4] = (site, p1, p2, p3), [n][3] weights (three-particle average). */
tgnh_status tgnh_harness_set_clusters(tgnh_handle h, int n, const int32_t* atoms, const double* dist);
tgnh_status tgnh_harness_shake_positions(tgnh_handle h, double tol, void* stream);    /* SHAKE on posDelta */
tgnh_status tgnh_harness_shake_velocities(tgnh_handle h, double tol, void* stream);   /* velocity stage on velm */
tgnh_status tgnh_harness_set_virtual_sites(tgnh_handle h, int n, const int32_t* atoms, const double* weights);
tgnh_status tgnh_harness_virtual_sites(tgnh_handle h, void* stream);
/* nsteps x { begin_kick, SHAKE, begin_move, virtual sites, harness force, end_kick, [TGNH: velocity stage], end_thermo };
 * with a table of tgnh_set_constraint_clusters (below), tgnh_apply_constraints behind SHAKE and tgnh_apply_velocity_constraints
 * behind the velocity stage -- with an empty one, the launches above and no other; with a table of tgnh_set_virtual_sites
 * (further below), tgnh_compute_virtual_sites behind the harness' virtual sites -- with an empty one, the launches above and no other */
tgnh_status tgnh_run_harness_constrained(tgnh_handle h, const void* x0, double k_drude, double k_tether,
                                         double tol, int nsteps, void* stream);

/* THE LIBRARY'S OWN CONSTRAINT STAGE, for a host that has no OpenMM behind it (the OpenMM glue keeps calling OpenMM's
 * applyConstraints / applyVelocityConstraints): every cluster solved directly on the device, one lane per cluster, with no iteration
 * to convergence.  It stands beside the harness call-outs above and does not replace them.
 *
 * tgnh_set_constraint_clusters(n, atoms, dist): clusters in the harness' canonical form -- [n][4] slot indices (-1 = unused) and
 * [n][6] distances for the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), 0 = unconstrained -- with ONE, TWO OR THREE constraints each:
 * a rigid three-site water, X-H, X-H2, X-H3.  The inverse masses are taken from the descriptor's masses, never from velm.  The
 * table replaces the one set before; n = 0 clears it.  The arrays are read before the call returns.  Every check runs before any
 * device work, so a host-only handle gives the same answers and the same count.  TGNH_ERR_ARG: n < 0 or a NULL array, an index out
 * of range, an atom listed twice in a cluster or in two clusters (two lanes would write one slot), a constraint whose pair names an
 * unused atom, a negative or non-finite distance, a cluster without any constraint.  TGNH_ERR_UNSUPPORTED, with the cluster's
 * number in tgnh_last_error(): more than three constraints in a cluster (leave it to an iterative solver -- the harness' takes
 * it), a constrained atom without mass.  THE DEGREES OF FREEDOM STAY WITH THE DESCRIPTOR'S CONSTRAINT LIST (num_constraints,
 * constraint_i / _j): this table changes nothing of tgnh_get_dof.  Not inside a stream capture (the table is uploaded synchronously).
 * tgnh_get_num_constraint_clusters: the clusters in force.
 *
 * With r_k = x(i_k) - x(j_k) the bond vector of constraint k before the move, w the inverse masses and c_kl the sum over the atoms
 * two constraints share of +-w (w_i + w_j for k = l), everything in fp64 in every precision:
 * tgnh_apply_constraints(tol): on posDelta, where the reference calls applyConstraints (Cu :363).  Multipliers lambda move atom i_k
 * by +lambda_k w_i r_k and atom j_k by -lambda_k w_j r_k.  EXACTLY FOUR Newton iterations from lambda = 0 on
 * sigma_k = |s_k(lambda)|^2 - d_k^2 (s_k: the bond vector after the move, of x + posDelta), each one K x K solve with the Jacobian
 * 2 (s_k . r_l) c_kl; x is posq (+ posq_correction in mixed precision).  The converged result is SHAKE's converged result.  Four
 * iterations reach fp64 rounding from displacements of a 1-2 fs step at 300 K drawn without regard to the constraints.
 * tgnh_apply_velocity_constraints(tol): on velm, where the reference calls applyVelocityConstraints (Cu :391).  Linear: ONE solve of
 * sum_l (r_k . r_l) c_kl mu_l = r_k . (v_i - v_j), then v_i -= mu_k w_i r_k, v_j += mu_k w_j r_k.  Clears the kinetic energies
 * carried under TGNH_FLAG_TRUST_STATE_CHANGED, as tgnh_harness_shake_velocities does.
 * `tol` does not steer the solve; it is the gate on the result, the harness' own: |sigma_k| <= 2 tol d_k^2, and
 * |r_k . (v_i - v_j)| / r_k^2 <= tol.  A cluster that misses it -- a NaN misses it -- sets status bit 1 (tgnh_get_status_flags), and
 * its result is stored all the same.  Only x, y, z of the clusters' atoms are written: w of posDelta and velm, every other slot,
 * posq and posq_correction stay bit for bit.  One launch each on `stream`, none with an empty table (TGNH_OK); neither call
 * synchronises, both can be captured into a hipGraph.  TGNH_ERR_STATE: a host-only handle, buffers not bound, (positions) no posDelta
 * bound.  tgnh_run_harness_constrained runs each of the two right after its harness counterpart -- the clusters of the two tables
 * are the caller's to keep disjoint. */
tgnh_status tgnh_set_constraint_clusters(tgnh_handle h, int n, const int32_t* atoms /* [n][4], -1 = unused */, const double* dist /* [n][6] */);
tgnh_status tgnh_get_num_constraint_clusters(tgnh_handle h, int* count);
tgnh_status tgnh_apply_constraints(tgnh_handle h, double tol, void* stream);            /* on posDelta: where Cu :363 calls out */
tgnh_status tgnh_apply_velocity_constraints(tgnh_handle h, double tol, void* stream);   /* on velm: where Cu :391 calls out */

/* THE LIBRARY'S OWN VIRTUAL-SITE STAGE, for a host that has no OpenMM behind it (the OpenMM glue keeps calling OpenMM's
 * computeVirtualSites): sites placed from their parents, and the forces that land on sites spread back over the parents, on the
 * device.  It stands beside the harness call-out above (three-particle averages, no way back for forces) and does not replace it.
 *
 * tgnh_set_virtual_sites(n, kind, atoms, params): kind[n] one of TGNH_SITE_*; atoms [n][4] = (site, p1, p2, p3) slots of the bound
 * arrays, p3 = -1 for a two-particle site (where it is not looked at); params [n][TGNH_SITE_PARAMS], of which a kind reads the first
 * 2, 3, 3 or 12.  With x1, x2, x3 the parents' positions and r1k = xk - x1, OpenMM's four kinds:
 *   TGNH_SITE_TWO_AVERAGE        w1, w2                       w1 x1 + w2 x2
 *   TGNH_SITE_THREE_AVERAGE      w1, w2, w3                   (w1 x1 + w2 x2) + w3 x3
 *   TGNH_SITE_OUT_OF_PLANE       w12, w13, wc                 x1 + w12 r12 + w13 r13 + wc (r12 x r13)
 *   TGNH_SITE_LOCAL_COORDINATES  wo[3], wx[3], wy[3], p[3]    o + p.x X + p.y Y + p.z Z, with o = sum wo x, X = normalise(sum wx x),
 *                                                             Z = normalise((sum wx x) x (sum wy x)), Y = Z x X
 * The table replaces the one set before; n = 0 clears it.  The arrays are read before the call returns; the rows may come in any
 * order.  Every check runs before any device work, so a host-only handle gives the same answers and the same count.  TGNH_ERR_ARG:
 * n < 0 or a NULL array, an unknown kind, an index out of range, a slot listed as a site twice, a parent repeated within a site, a
 * parent that is itself a site, p3 = -1 for a kind that needs three parents, a parameter (of those the kind reads) that is not
 * finite, local-coordinates weights with |sum wo - 1|, |sum wx| or |sum wy| above 1e-6 (OpenMM's own gate).  TGNH_ERR_UNSUPPORTED,
 * with the site's number in tgnh_last_error(): a site whose mass in the descriptor is not zero, a site that is a member of a Drude
 * pair.  Not inside a stream capture (the table is uploaded synchronously).  tgnh_get_num_virtual_sites: the sites in force.
 * A refused table leaves the one in force as it was, and so does a table whose upload fails (TGNH_ERR_HIP): the new one is built
 * aside and replaces the old one only when it is complete.
 *
 * Everything below in fp64 in every precision.  A parent's position is posq, + posq_correction in mixed precision, as
 * tgnh_get_drude_statistics defines it.  For the two average kinds every operation is rounded on its own (no fused multiply-add), in
 * the order written above, per component.
 * tgnh_compute_virtual_sites: where the reference calls computeVirtualSites (Cu :377).  Stored as the harness stores its sites:
 * mixed precision the fp32 value and, in posq_correction, the residual; single precision rounded once.  Only x, y, z of the sites'
 * slots are written: posq.w and posq_correction.w, every other slot, velm, posDelta and the force buffer stay bit for bit.
 * tgnh_distribute_virtual_site_forces(force): right after the force call-out.  `force` is int64 [3*padded] fixed point x 2^32,
 * planes x|y|z -- normally the bound buffer.  Per site f = F_site / 2^32; each parent's share is the transpose of the placement's
 * Jacobian, at the current parent positions, applied to f:
 *   averages            w_m f
 *   out of plane        f2 = w12 f + wc (r13 x f), f3 = w13 f - wc (r12 x f), f1 = f - f2 - f3
 *   local coordinates   through the two normalisations and the cross product (csrc/tgnh_virtual_sites.hip writes them out)
 * Each component of each share is converted on its own, llrint(c * 4294967296.0), and added to the parent's entry as an integer: the
 * result is a function of the inputs alone -- not of grid, order or device -- and no atomic operation touches the buffer.  The
 * sites' own entries are read and left as they are: TWO CALLS ADD TWICE.  Call it once per force evaluation.
 * One launch each on `stream`, none with an empty table (TGNH_OK); neither call synchronises, both can be captured into a hipGraph.
 * Both may run at any time with respect to kicks a step still owes (tgnh_get_pending_state): sites have no mass, and nothing the
 * handle carries depends on their positions.  A degenerate local-coordinates frame (sum wx x parallel to sum wy x) stores the
 * non-finite numbers it produces; there is no status bit for it.  TGNH_ERR_STATE: a host-only handle, buffers not bound,
 * (distribute) force is NULL.  tgnh_run_harness_constrained runs the placement right after the harness' -- the sites of the two
 * tables are the caller's to keep disjoint. */
enum { TGNH_SITE_TWO_AVERAGE = 0, TGNH_SITE_THREE_AVERAGE = 1, TGNH_SITE_OUT_OF_PLANE = 2, TGNH_SITE_LOCAL_COORDINATES = 3 };
#define TGNH_SITE_PARAMS 12
tgnh_status tgnh_set_virtual_sites(tgnh_handle h, int n, const int32_t* kind /* [n] */, const int32_t* atoms /* [n][4], p3 = -1: two parents */,
                                   const double* params /* [n][TGNH_SITE_PARAMS] */);
tgnh_status tgnh_get_num_virtual_sites(tgnh_handle h, int* count);
tgnh_status tgnh_compute_virtual_sites(tgnh_handle h, void* stream);                             /* where Cu :377 calls out */
tgnh_status tgnh_distribute_virtual_site_forces(tgnh_handle h, void* force, void* stream);       /* right after the force call-out */

/* THE LIBRARY'S OWN DRUDEFORCE, for a host that has no OpenMM behind it (inside OpenMM the System's DrudeForce keeps acting, and the
 * glue calls none of this): the springs that hold the Drude particles, their anisotropy, the Thole-screened pairs and the energy, on
 * the device.  It stands beside the harness forces (tgnh_harness_force: a bench workload with a tether; tgnh_harness_water_force:
 * testWater's one isotropic spring per molecule) and replaces neither.  Coulomb and Lennard-Jones forces are not here: THE LIBRARY'S OWN NONBONDED FORCE below has them.
 *
 * tgnh_set_drude_force: OpenMM's DrudeForce::addParticle / addScreenedPair as a table.  particles [n][5] = (p, p1, p2, p3, p4) slots
 * of the bound arrays, -1 = none for p2..p4; params [n][4] = (charge e, polarizability nm^3, aniso12, aniso34); screened
 * [num_screened][2] = rows (i, j) of that table; thole [num_screened].  ROW k NAMES THE DESCRIPTOR'S PAIR k: p == pair_drude[k],
 * p1 == pair_parent[k] and n == num_pairs (tgnh_desc takes the pairs "in DrudeForce order" for this).  The table replaces the one set
 * before; n = 0 clears it.  The arrays are read before the call returns.  Every check runs before any device work, so a host-only
 * handle gives the same answers and the same counts (tgnh_get_num_drude_force_terms).  Not inside a stream capture: the table, its
 * inverse and the energy's scratch are uploaded and allocated here, synchronously, and never later.
 * The constants are formed on the host, once, in fp64, with C = ONE_4PI_EPS0 = 138.935456 kJ nm / (mol e^2):
 *   a1 = aniso12 if p2 != -1, else 1;   a2 = aniso34 if p3 != -1 and p4 != -1, else 1;   a3 = 3 - a1 - a2
 *   k3 = C q^2 / (alpha a3);   k1 = C q^2 / (alpha a1) - k3;   k2 = C q^2 / (alpha a2) - k3     (k1, k2: 0 where the row has no such axis)
 *   per screened pair:  a = thole / (alpha_i alpha_j)^(1/6),   K = C q_i q_j
 * (This mapping from polarizability and aniso values to k1, k2, k3 is believed to be OpenMM's; OpenMM was not at hand to check
 * against.  The reference embeds DrudeForce's two kernels with k1, k2, k3 handed in -- the per-term forms below are theirs -- and its
 * testWater uses the isotropic case only, k3 = C q^2 / alpha.)
 * TGNH_ERR_ARG, the row's or the pair's number in tgnh_last_error(): n neither 0 nor num_pairs, a NULL array, num_screened < 0; a
 * row that does not name its pair; an index out of range; p2 equal to p or p1, p3 == p4, exactly one of p3 and p4 equal to -1; a
 * charge that is not finite; a polarizability that is not finite or <= 0; an aniso value (of those the row reads) that is not
 * finite or <= 0, or a3 <= 0; a screened pair that names a row out of range, one row twice, or a pair of rows listed before, in
 * either order; a thole that is negative or not finite.  A refused table leaves the one in force as it was, and so does a table whose
 * upload fails (TGNH_ERR_HIP): the new one is built aside and replaces the old one only when it is complete.
 *
 * tgnh_compute_drude_force(force, want_energy).  Everything in fp64 in every precision.  A position x(i) is posq, + posq_correction
 * in mixed precision, as tgnh_get_drude_statistics defines it.  Charges come from the table, never from posq.w.  The terms:
 *   per row, delta = x(p) - x(p1):
 *     the isotropic spring          t = k3 delta;   p: -t,  p1: +t;   E = 1/2 k3 |delta|^2
 *     the first axis (p2 != -1)     d = x(p1) - x(p2), e = d / |d|, s = e . delta, f1 = (k1 s) e, f2 = (k1 s / |d|)(delta - s e);
 *                                   p: -f1,  p1: f1 - f2,  p2: f2;   E = 1/2 k1 s^2
 *     the second axis (p3, p4)      d = x(p3) - x(p4), the same e, s, f1, f2 with k2;   p: -f1,  p1: +f1,  p3: -f2,  p4: +f2;   E = 1/2 k2 s^2
 *   per screened pair of rows (i, j) its four site pairs (first in {p_i, p1_i}, second in {p_j, p1_j}), each a term of its own,
 *   sigma = +1 for Drude-Drude and parent-parent, -1 for the two mixed ones; delta = x(first) - x(second), r = |delta|, u = a r,
 *   S = 1 - (1 + u/2) exp(-u):
 *     E = sigma K S / r;   first: delta sigma K (S / r - 1/2 (1 + u) exp(-u) a) / r^2,   second: its negative
 * Each component of each particle's share of each term is converted on its own, llrint(c * 4294967296.0), and added to the particle's
 * entry as an integer (tgnh_distribute_virtual_site_forces' rule): the result is a function of the inputs alone -- not of grid,
 * order, device or step path -- and no atomic operation touches the buffer.  The isotropic shares are formed without fused
 * multiply-add, every operation rounded on its own as written: bit for bit what a numpy restatement gives.  sqrt, exp and the
 * divisions are the IEEE ones.  A thole of 0 gives S = 0 and shares of exactly 0.
 * `force` is int64 [3*padded] fixed point x 2^32, planes x|y|z -- normally the bound buffer.  The call ADDS: two calls add twice.
 * Padding and slots in no term are neither read nor written; positions, velm and posDelta are only read or not touched at all.
 * A pair at r = 0 or an axis of length 0 stores the non-finite numbers it produces; there is no status bit for it.
 * One launch on `stream` (one lane per receiving slot over the table inverted at set time; a term is recomputed by every particle
 * that receives from it), none with an empty table (TGNH_OK).  It does not synchronise and can be captured into a hipGraph.  It is
 * not a tgnh_state_changed, and may run at any time with respect to kicks a step still owes (tgnh_get_pending_state), as the site
 * calls may: it reads positions, and only velm ever lags.  TGNH_ERR_STATE: a host-only handle, buffers not bound, force is NULL.
 * Follows tgnh_get_status_flags' rule for sticky failures.
 *
 * THE ENERGY.  want_energy != 0: the same launch also leaves a row of partial sums {springs, screened pairs} per work-group, in
 * scratch allocated at set time.  tgnh_get_drude_energy enqueues the one-work-group sum of the rows, synchronises `stream` and
 * returns out[0] = the springs' energy (isotropic and both axes), out[1] = the screened pairs', kJ/mol.  Each term is counted by
 * exactly one lane: a row by the lane of its p, a screened pair (its four site pairs, added in the order Drude_i-Drude_j,
 * Drude_i-parent_j, parent_i-Drude_j, parent_i-parent_j) by the lane of row i's p.  No floating-point atomic; the grid is a function
 * of the number of receiving slots alone and every order of additions is fixed by it, so the same positions give the same bits from
 * any handle over the same slots and the same table, tiled or TGNH_FLAG_GATHER, TGNH or DUALNH, asked once or twice.
 * TGNH_ERR_STATE: no tgnh_compute_drude_force with want_energy since the table was set -- a launch that was only RECORDED into a
 * stream capture does not count (nothing has run; the replayed graph fills the rows, and an eager want_energy launch before or after
 * the capture opens the query) --; a host-only handle, buffers not bound.
 * TGNH_ERR_ARG: out is NULL.
 * SHARDED RUNS: shards are whole molecules; every rank hands over the rows of its own pairs with local indices, and a
 * term that names a particle outside the shard is refused by the index check.  Nothing is exchanged: the forces are local and the
 * two energies are additive over ranks. */
tgnh_status tgnh_set_drude_force(tgnh_handle h, int n, const int32_t* particles /* [n][5]: p, p1, p2, p3, p4; -1 = none for p2..p4 */,
                                 const double* params /* [n][4]: charge, polarizability, aniso12, aniso34 */,
                                 int num_screened, const int32_t* screened /* [num_screened][2]: rows of the table above */,
                                 const double* thole /* [num_screened] */);
tgnh_status tgnh_get_num_drude_force_terms(tgnh_handle h, int* rows, int* screened_pairs);
tgnh_status tgnh_compute_drude_force(tgnh_handle h, void* force, int want_energy, void* stream);    /* in the force call-out */
tgnh_status tgnh_get_drude_energy(tgnh_handle h, void* stream, double out[2] /* springs, screened pairs */);   /* synchronises */

/* THE LIBRARY'S OWN BONDED FORCES, for a host that has no OpenMM behind it (inside OpenMM the System's forces keep acting, and the glue
 * calls none of this): OpenMM's HarmonicBondForce, HarmonicAngleForce and PeriodicTorsionForce and their energies, on the device -- the
 * covalent half of an intramolecular force field beside the DrudeForce above.  Coulomb and Lennard-Jones forces are not here.
 * PERIODIC IMAGES ARE NOT APPLIED: a term acts along the stored positions, and molecules are kept whole by tgnh_wrap_molecules.
 *
 * tgnh_set_bonded_forces: three tables.  bond_particles [nb][2] = (p1, p2) slots of the bound arrays, bond_params [nb][2] = (length nm,
 * k kJ/mol/nm^2); angle_particles [na][3] = (p1, p2, p3), p2 the centre, angle_params [na][2] = (angle rad, k kJ/mol/rad^2);
 * torsion_particles [nt][4] = (p1, p2, p3, p4), torsion_periodicity [nt], torsion_params [nt][2] = (phase rad, k kJ/mol).  The three
 * replace the ones set before, together; all three counts 0 clears them.  The arrays are read before the call returns.  Every check
 * runs before any device work, so a host-only handle gives the same answers and the same counts (tgnh_get_num_bonded_terms: out[3] =
 * bonds, angles, torsions).  Not inside a stream capture: the tables, their inverse and the energy's scratch are uploaded and allocated
 * here, synchronously, and never later.  cos(phase) and sin(phase) are formed here, once, in fp64.
 * TGNH_ERR_ARG, the kind and the row's number in tgnh_last_error() ("bond 5", "angle 0", "torsion 17"): a negative count; a NULL array
 * with a positive count; an index out of range; a particle named twice within one term; a length, angle, phase or k that is not
 * finite; a length < 0; an angle outside [0, pi]; a periodicity < 1.  TGNH_ERR_UNSUPPORTED: a periodicity > 12; more entries
 * (2 nb + 3 na + 4 nt) than the inverted table's 32-bit offsets take -- decided from the counts alone, before any row is read.
 * DUPLICATE TERMS on the same particles are allowed, unlike screened pairs (force fields stack several periodicities on one dihedral),
 * and a row with k = 0 is legal and contributes shares of exactly 0.  Refused tables leave the ones in force as they were, and so do
 * tables whose upload fails (TGNH_ERR_HIP): the new ones are built aside and replace the old ones only when they are complete.
 *
 * tgnh_compute_bonded_forces(force, want_energy).  Everything in fp64 in every precision.  A position x(i) is posq, + posq_correction
 * in mixed precision, as tgnh_get_drude_statistics defines it.  Every operation is rounded on its own, in the order written (no fused
 * multiply-add); sqrt and the divisions are the IEEE ones.  The terms:
 *   bond (p1, p2; r0, k):   d = x(p2) - x(p1), r = sqrt((dx^2 + dy^2) + dz^2), c = (k (r - r0)) / r;
 *                           p1: +c d,  p2: -c d;   E = (0.5 k (r - r0)) (r - r0)
 *   angle (p1, p2, p3; t0, k):   a = x(p1) - x(p2), b = x(p3) - x(p2), c = a x b, s = max(|c|, 1e-6) (OpenMM's floor: a collinear angle
 *                           with t0 = pi gives exactly zero, finite shares), t = atan2(|c|, a . b) (not acos, which loses half the
 *                           digits near 0 and pi), g = k (t - t0);
 *                           F1 = (g / ((a . a) s)) (c x a),  F3 = (g / ((b . b) s)) (b x c),  F2 = -(F1 + F3), each component formed from
 *                           the fp64 F1 and F3 and then converted;   p1: F1,  p2: F2,  p3: F3;   E = (0.5 g) (t - t0)
 *   torsion (p1, p2, p3, p4; n, phi0, k):   v0 = x(p1) - x(p2), v1 = x(p3) - x(p2), v2 = x(p3) - x(p4), c0 = v0 x v1, c1 = v1 x v2,
 *                           l = sqrt(v1 . v1), X = c0 . c1, Y = l (v0 . c1), hyp = sqrt(X^2 + Y^2), cos phi = X / hyp, sin phi = Y / hyp
 *                           (the IUPAC sign: cis is 0, trans is pi).  No trigonometric call on the device: (C_1, S_1) = (cos phi, sin phi),
 *                           C_(m+1) = C_m cos phi - S_m sin phi, S_(m+1) = S_m cos phi + C_m sin phi up to m = n.
 *                           E = k (1 + (C_n cos phi0 + S_n sin phi0));   g = dE/dphi = -(k n) (S_n cos phi0 - C_n sin phi0);
 *                           F1 = (-g l / (c0 . c0)) c0,  F4 = (g l / (c1 . c1)) c1,
 *                           s = ((v0 . v1) / (v1 . v1)) F1 - ((v2 . v1) / (v1 . v1)) F4,  F2 = s - F1,  F3 = -s - F4;   p1..p4: F1..F4
 * (The angle and torsion shares were checked against central finite differences of the energies above in fp80,
 * tests/test_bonded_forces.py; they are -dE/dx.)
 * Each component of each particle's share of each term is converted on its own, llrint(c * 4294967296.0), and added to the particle's
 * entry as an integer (tgnh_compute_drude_force's rule): the result is a function of the inputs alone -- not of grid, order, device
 * or step path -- and no atomic operation touches the buffer.  The bond shares are bit for bit what a numpy restatement gives.
 * `force` is int64 [3*padded] fixed point x 2^32, planes x|y|z -- normally the bound buffer.  The call ADDS: two calls add twice.
 * Padding and slots in no term are neither read nor written; positions, velm and posDelta are only read or not touched at all.
 * A degenerate torsion (c0 or c1 of length 0) or a bond of length 0 stores the non-finite numbers it produces; there is no status
 * bit for it, as for a DrudeForce axis of length 0.
 * One launch on `stream` (one lane per receiving slot over the tables inverted at set time, bonds numbered first, then angles, then
 * torsions; a term is recomputed by every particle that receives from it), none with empty tables (TGNH_OK).  It does not synchronise
 * and can be captured into a hipGraph.  It is not a tgnh_state_changed, and may run at any time with respect to kicks a step still
 * owes (tgnh_get_pending_state), as tgnh_compute_drude_force may.  TGNH_ERR_STATE: a host-only handle, buffers not bound, force is
 * NULL.  Follows tgnh_get_status_flags' rule for sticky failures.
 *
 * THE ENERGY.  want_energy != 0: the same launch also leaves a row of partial sums {bonds, angles, torsions} per work-group, in scratch
 * allocated at set time.  tgnh_get_bonded_energy enqueues the one-work-group sum of the rows, synchronises `stream` and returns
 * out[0] = the bonds' energy, out[1] = the angles', out[2] = the torsions', kJ/mol.  Each term is counted by exactly one lane, the
 * lane of its p1.  No floating-point atomic; the grid is a function of the number of receiving slots alone and every order of
 * additions is fixed by it, so the same positions give the same bits from any handle over the same slots and the same tables, tiled
 * or TGNH_FLAG_GATHER, TGNH or DUALNH, asked once or twice.
 * TGNH_ERR_STATE: no tgnh_compute_bonded_forces with want_energy since the tables were set -- a launch that was only RECORDED into a
 * stream capture does not count (nothing has run; the replayed graph fills the rows, and an eager want_energy launch before or after
 * the capture opens the query) --; a host-only handle, buffers not bound.  TGNH_ERR_ARG: out is NULL.
 * SHARDED RUNS: shards are whole molecules; every rank hands over its own terms with local indices, and a term that
 * names a particle outside the shard is refused by the index check.  Nothing is exchanged: the forces are local and the three
 * energies are additive over ranks. */
tgnh_status tgnh_set_bonded_forces(tgnh_handle h,
    int num_bonds,    const int32_t* bond_particles    /* [nb][2] */, const double* bond_params    /* [nb][2]: length nm, k kJ/mol/nm^2 */,
    int num_angles,   const int32_t* angle_particles   /* [na][3], p2 the centre */, const double* angle_params /* [na][2]: angle rad, k kJ/mol/rad^2 */,
    int num_torsions, const int32_t* torsion_particles /* [nt][4] */, const int32_t* torsion_periodicity /* [nt] */,
                      const double* torsion_params     /* [nt][2]: phase rad, k kJ/mol */);
tgnh_status tgnh_get_num_bonded_terms(tgnh_handle h, int out[3]);
tgnh_status tgnh_compute_bonded_forces(tgnh_handle h, void* force, int want_energy, void* stream);   /* ADDS; one launch; capturable */
tgnh_status tgnh_get_bonded_energy(tgnh_handle h, void* stream, double out[3] /* bonds, angles, torsions */);   /* synchronises */

/* THE LIBRARY'S OWN NONBONDED FORCE, for a host that has no OpenMM behind it (inside OpenMM the System's NonbondedForce keeps acting, and
 * the glue calls none of this): Coulomb with a reaction field and Lennard-Jones between all particles inside a cutoff of a rectangular
 * periodic box, and OpenMM's exceptions -- the intermolecular half of a force field beside the DrudeForce and the bonded forces above.
 * The definitions are OpenMM's NonbondedForce with CutoffPeriodic, recalled from its published documentation, as oracle/water_ff.c
 * restates them; OpenMM was not at hand to check against.  Lattice-summed electrostatics: EWALD SUMMATION below, switched on by a call
 * of its own on top of this table.  NOT BUILT: PME, the switching function, the long-range dispersion correction, triclinic cells,
 * sharded pairs, a Verlet list with a skin (the cells are rebuilt by every call, so the call stays stateless).
 *
 * tgnh_set_nonbonded_force.  desc->particles [n][3] = (charge e, sigma nm, epsilon kJ/mol), one row per slot of the bound arrays:
 * charges come from this table, posq.w is neither read nor written.  exception_particles [ne][2] = (p1, p2), exception_params [ne][3] =
 * (chargeProd e^2, sigma nm, epsilon kJ/mol).  The table replaces the one set before; desc == NULL or num_particles == 0 clears it.  The
 * arrays are read before the call returns.  Every check runs before any device work, so a host-only handle gives the same answers and
 * the same counts (tgnh_get_num_nonbonded_terms: out[3] = particles, exceptions, of which evaluated).  Not inside a stream capture: the
 * tables, the exclusion list of every slot (ascending), the inverse of the evaluated exceptions and every per-slot buffer are uploaded
 * and allocated here, synchronously.  krf and crf are formed here, once, in fp64, each operation rounded on its own:
 *   krf = ((1 / ((rc rc) rc)) (eps - 1)) / (2 eps + 1)        crf = ((1 / rc) (3 eps)) / (2 eps + 1)
 * TGNH_ERR_ARG, with "particle 7" or "exception 3" in tgnh_last_error(): a struct_size that is not sizeof(tgnh_nonbonded_desc);
 * num_particles that is not the handle's slot count; a negative count; a NULL array with a positive count; a parameter that is not
 * finite; sigma < 0 or epsilon < 0; a cutoff that is not finite or <= 0; a dielectric that is not finite or < 1; an exception index out
 * of range; an exception with p1 == p2; the same pair in two exception rows (the later row is named).  TGNH_ERR_UNSUPPORTED: any method
 * but TGNH_NB_CUTOFF_PERIODIC; a handle that is one shard of several (a hook, RCCL or the mailboxes are attached): pairs cross shards
 * and nothing is exchanged here; 2 ne beyond 32-bit offsets (decided from the count alone).  A refused table leaves the one in force as
 * it was, and so does one whose upload fails (TGNH_ERR_HIP): the new one is built aside and swapped in when it is complete.
 *
 * tgnh_compute_nonbonded_force(force, want_energy).  Everything in fp64 in every precision.  x(i) is posq, + posq_correction in mixed
 * precision, as tgnh_get_drude_statistics defines it.  Every operation is rounded on its own, in the order written (no fused
 * multiply-add); sqrt and the divisions are the IEEE ones; rint rounds to nearest, ties to even.  K = 138.935456.  L is the box's edge
 * along the component, rc the cutoff.
 * PAIRS.  Every unordered pair {a, b} of slots that no exception row names gets a term.  For the share of particle a, b the other
 * one, per component k:
 *   d_k  = x_k(a) - x_k(b)
 *   t_k  = d_k / L_k
 *   t_k  = rint(t_k)                       (not floor(t + 0.5): rint is odd, so the pair's two lanes hold exactly negated d)
 *   t_k  = L_k t_k
 *   d_k  = d_k - t_k
 * (The device skips the division where the result of these four lines is known exactly: |d_k| <= 0.49 L_k leaves d_k as it is, since
 * rint gives 0; 0.51 L_k <= |d_k| <= 1.49 L_k gives d_k - copysign(L_k, d_k), since rint gives +-1 and L (+-1) is +-L.  The margins
 * of 0.01 keep the rounded quotient off the ties at 0.5 and 1.5.  Everything else, a NaN included, takes the four lines: same bits.)
 * then
 *   r2   = (dx dx + dy dy) + dz dz         the pair is skipped unless r2 < rc rc
 *   r    = sqrt(r2)
 *   inv  = 1 / r
 *   qq   = K (q_a q_b)                     (the charges' product first: it commutes, so both lanes hold the same bits, and a
 *                                           permutation of the slots permutes the result; (K q_a) q_b would do neither)
 *   sig  = 0.5 (sigma_a + sigma_b)
 *   e4   = 4 sqrt(epsilon_a epsilon_b)
 *   s2   = (sig sig) / r2
 *   s6   = (s2 s2) s2
 *   s12  = s6 s6
 *   dc   = qq ((2 krf) r - inv inv)        the Coulomb part of dE/dr
 *   dl   = (e4 (6 s6 - 12 s12)) inv        the Lennard-Jones part
 *   c    = -((dc + dl) inv)
 *   particle a receives llrint((c d_k) 4294967296.0) per component, added as an integer
 *   E_C  = qq ((inv + krf r2) - crf)       E_LJ = e4 (s12 - s6)
 * EXCEPTIONS.  Every pair an exception row names is left out of the above.  A row with chargeProd != 0 or epsilon != 0 is evaluated on
 * its own, with no cutoff, no reaction field and NO PERIODIC IMAGE (molecules are whole: the bonded section's rule); any other row is a
 * pure exclusion.  For the share of particle a of the row, b the other one:
 *   d_k  = x_k(a) - x_k(b);   r2, r, inv as above;   qq = K chargeProd;   e4 = 4 epsilon;   s2 = (sigma sigma) / r2;   s6, s12 as above
 *   dc   = qq (-(inv inv));   dl = (e4 (6 s6 - 12 s12)) inv;   c = -((dc + dl) inv);   llrint((c d_k) 4294967296.0) as above
 *   E_C  = qq inv             E_LJ = e4 (s12 - s6)
 * Every contribution is converted on its own and added as an integer, so the change of the force buffer is a function of positions,
 * box and tables alone -- not of cell order, grid or path --, a numpy restatement gives it bit for bit (tests/test_nonbonded.py), and a
 * pair's two shares cancel exactly.  `force` is int64 [3*padded] fixed point x 2^32, planes x|y|z -- normally the bound buffer.  The
 * call ADDS: two calls add twice.  No atomic operation touches the buffer.  Padding is neither read nor written; positions, velm and
 * posDelta are only read or not touched at all.  Two particles that no exception names at r = 0 store the non-finite numbers that come
 * out; there is no status bit for it.
 * THE CELLS.  nc_k = max(1, floor(L_k / (1.001 rc))) cells per edge (the 1.001 keeps a one-ulp misassignment at a cell face from hiding
 * a pair inside the cutoff); a slot's cell per component is s = x / L, s = s - floor(s), min((int)(s nc), nc - 1): positions far outside
 * the box and negative ones are legal.  More than 2^24 cells: TGNH_ERR_UNSUPPORTED.  LAUNCHES: one memset and five kernels a call --
 * cell, scan, place, rank, pairs -- and a sixth when some exception is evaluated; the numbers do not depend on n.  None with no table
 * set (TGNH_OK).  The call does not synchronise and can be captured into a hipGraph; a graph bakes in the box it was recorded with.
 * The per-cell buffers grow at the first call whose box needs more cells than they hold: on a capturing stream that call returns
 * TGNH_ERR_STATE and asks for one call outside the capture (the frame rule); growing them invalidates graphs recorded before.
 * TGNH_ERR_STATE: a host-only handle, buffers not bound, force is NULL, no box set.  TGNH_ERR_UNSUPPORTED: a box with a non-zero
 * off-diagonal component; a cutoff above half the shortest edge; a sharded handle.  Follows tgnh_get_status_flags' rule for sticky
 * failures.  It is not a tgnh_state_changed.
 *
 * THE ENERGY.  want_energy != 0: the pair launch also leaves a row {E_C, E_LJ} per work-group -- a lane counts a pair only when the
 * other slot is larger than its own, and adds in traversal order: neighbour cells z, then y, then x from c - 1 upwards, members in
 * (cell, slot) order -- and the exception launch a row per work-group, the lane of a row's p1 counting it.  tgnh_get_nonbonded_energy
 * enqueues the one-work-group sum, synchronises `stream` and returns out[0] = the pairs' Coulomb energy with the reaction field,
 * out[1] = the pairs' Lennard-Jones energy, out[2], out[3] = the evaluated exceptions' Coulomb and Lennard-Jones energy, kJ/mol.  No
 * floating-point atomic: the same positions, box and tables give the same bits from any handle over the same slots, tiled or
 * TGNH_FLAG_GATHER, TGNH or DUALNH, asked once or twice.  TGNH_ERR_STATE: no tgnh_compute_nonbonded_force with want_energy since the
 * table was set or since the per-cell buffers last grew (a launch that was only recorded into a stream capture does not count); a host-only handle, buffers not bound.
 * TGNH_ERR_ARG: out is NULL. */
enum { TGNH_NB_NO_CUTOFF = 0, TGNH_NB_CUTOFF_NONPERIODIC = 1, TGNH_NB_CUTOFF_PERIODIC = 2 };   /* OpenMM's numbering */
typedef struct tgnh_nonbonded_desc {
    uint32_t struct_size;             /* sizeof(tgnh_nonbonded_desc); anything else: TGNH_ERR_ARG */
    int32_t method;                   /* only TGNH_NB_CUTOFF_PERIODIC is taken */
    double cutoff;                    /* nm */
    double reaction_field_dielectric; /* OpenMM's default 78.3 */
    int32_t num_particles;
    const double* particles;          /* [n][3] charge e, sigma nm, epsilon kJ/mol: one row per slot of the bound arrays */
    int32_t num_exceptions;
    const int32_t* exception_particles;   /* [ne][2] */
    const double* exception_params;   /* [ne][3] chargeProd, sigma, epsilon */
} tgnh_nonbonded_desc;
tgnh_status tgnh_set_nonbonded_force(tgnh_handle h, const tgnh_nonbonded_desc* d);      /* d == NULL or num_particles == 0 clears */
tgnh_status tgnh_get_num_nonbonded_terms(tgnh_handle h, int out[3]);                    /* particles, exceptions, of which evaluated */
tgnh_status tgnh_compute_nonbonded_force(tgnh_handle h, void* force, int want_energy, void* stream);   /* ADDS; capturable */
tgnh_status tgnh_get_nonbonded_energy(tgnh_handle h, void* stream, double out[4]);      /* pair Coulomb (with reaction field), pair LJ, exception Coulomb, exception LJ; synchronises */

/* EWALD SUMMATION on top of the table above: OpenMM's `Ewald` method, an explicit sum over reciprocal vectors with no FFT.  The cost is
 * O(n M), M the number of reciprocal vectors: it suits boxes of up to a few ten thousand slots, and is what PME (PARTICLE-MESH EWALD
 * below) is checked against.  tgnh_set_nonbonded_force's descriptor, checks and texts are unchanged (methods 3, 4, 5 are refused there
 * as before): Ewald is switched on by tgnh_set_nonbonded_ewald while a CutoffPeriodic table is in force, and every
 * tgnh_set_nonbonded_force, a clearing one included, drops the setting again.  With no Ewald setting nothing below is allocated or
 * launched, and tgnh_compute_nonbonded_force is what it was, launch for launch and bit for bit.
 *
 * tgnh_set_nonbonded_ewald(desc).  desc == NULL: back to the reaction field.  Every check runs before any device work, so a host-only
 * handle gives the same answers.  TGNH_ERR_STATE: no nonbonded table is set.  TGNH_ERR_ARG, with the reason in tgnh_last_error(): a
 * struct_size that is not sizeof(tgnh_ewald_desc); an alpha that is not finite or <= 0; a kmax component < 0 or > 255.
 * TGNH_ERR_UNSUPPORTED: M > 2^20 (tgnh_set_nonbonded_pme is for that).  A refused call leaves whatever was in force untouched.  The reciprocal vectors are the (nx, ny, nz)
 * != 0 with |n_d| <= kmax_d whose first non-zero component is positive, a half space of
 *   M = ((2 kmax_x + 1)(2 kmax_y + 1)(2 kmax_z + 1) - 1) / 2
 * vectors, stored in the order nx, then ny, then nz, ascending; kmax = (0, 0, 0) is legal and means no reciprocal part.  Not inside a
 * stream capture: the table of vectors, the partial-sum rows (sized from n and M), the receiver table of the exclusion correction and
 * the set-time constants are allocated and uploaded here, synchronously, so that the compute call never grows anything because of
 * Ewald.  The call has no stream of its own: it returns TGNH_ERR_STATE when the stream of the handle's last
 * tgnh_compute_nonbonded_force is capturing; a capture on a stream this handle has not seen is the caller's to avoid.  Formed here,
 * once, in fp64, each operation rounded on its own (pi = 3.14159265358979323846, sqrt the IEEE one):
 *   tsp    = (2 alpha) / sqrt(pi)                 a4 = 4 (alpha alpha)
 *   E_self = -((K (alpha / sqrt(pi))) sum q q)    the sum over the table's charges in slot order
 *   bgn    = ((pi K) (Q Q)) / (2 (alpha alpha))   Q the table's net charge, summed in slot order
 * tgnh_get_nonbonded_ewald: the setting in force (out->struct_size 0: off) and M.
 *
 * With Ewald on, tgnh_compute_nonbonded_force(force, want_energy) adds the terms below.  Everything in fp64 in every precision, every
 * operation rounded on its own in the order written; x(i), K, L as above; V = (Lx Ly) Lz; erfc, erf, exp and sincospi are the device
 * library's (a restatement with another library's cannot give the same bits: tests/test_ewald.py measures how far one is off).
 * DIRECT SPACE.  The pair launch: the same pairs, minimum image, cutoff and Lennard-Jones lines as PAIRS above; the Coulomb part is
 *   ar   = alpha r
 *   ec   = erfc(ar)
 *   g    = exp(-(ar ar))
 *   dc   = qq (-((ec inv + tsp g) inv))
 *   E_C  = qq (ec inv)
 * Both lanes of a pair hold the same r bits, hence the same ec and g: the pair's two integer shares still cancel exactly.
 * EXCLUSION CORRECTION.  Every exception row (p1, p2), evaluated or not, whose particles' table charges have a non-zero product; no
 * cutoff and no periodic image (the bonded rule).  For the share of particle a of the row, b the other one:
 *   d_k  = x_k(a) - x_k(b);   r2 = (dx dx + dy dy) + dz dz;   qq = K (q_p1 q_p2)
 *   r2 == 0 (a Drude particle on its parent): no force, E = -(qq tsp)
 *   otherwise r = sqrt(r2), inv = 1 / r, ar = alpha r
 *   ef   = erf(ar)
 *   g    = exp(-(ar ar))
 *   dc   = qq ((ef inv - tsp g) inv)
 *   c    = -(dc inv)
 *   particle a receives llrint((c d_k) 4294967296.0) per component
 *   E    = -(qq (ef inv))
 * One lane per receiving slot over the rows inverted at set time, as the evaluated exceptions; those stay as they are.
 * RECIPROCAL SPACE.  For slot j: s_d = x_d / L_d, then s_d = s_d - floor(s_d) (the cell build's two lines); for vector m = (nx, ny, nz):
 *   t     = (nx sx + ny sy) + nz sz               the phase in turns
 *   (sin, cos) = sincospi(2 t)
 *   C_m   = sum_j q_j cos      S_m = sum_j q_j sin        over parts of 4096 consecutive slots: within a part in slot order from 0,
 *                                                         then the parts in order from 0
 *   k_d   = ((2 pi) n_d) / L_d      k2 = (kx kx + ky ky) + kz kz      A_m = exp(-(k2 / a4)) / k2
 *   w_im  = (A_m C_m) sin_im - (A_m S_m) cos_im           g_d = sum_m k_md w_im    in the table's order, from 0
 *   slot i receives llrint((((8 (pi K)) / V) q_i) g_d 4294967296.0) once per component; a slot with charge 0 receives nothing
 *   E_rec = ((4 (pi K)) / V) sum_m A_m (C_m C_m + S_m S_m)      summed as the other energies' rows are
 * E_bg = -(bgn / V), formed on the device with the box of the call, as A_m and k_m are: a box that changes between calls needs no
 * reset, and a captured call stays correct for the box it recorded.
 * ORDER.  No floating-point atomic anywhere, no atomic on the force buffer; every sum's order depends on n, M and the tables alone,
 * not on the device or the grid: the same positions, box and tables give the same bits from a tiled, a TGNH_FLAG_GATHER and a DUALNH
 * handle, asked once or twice, run eagerly or replayed from a graph.  The direct and exclusion parts stay a function of positions,
 * box and tables alone, and a permutation of the slots permutes their bits.  The reciprocal part is NOT permutation-invariant bit for
 * bit: C_m and S_m are summed in slot order.
 * LAUNCHES.  The memset and five or six kernels of the call stay; Ewald adds one kernel when some exception row has charged partners
 * and three when M > 0 (sum, finalise, force): a function of the tables alone, never of n.  The call stays capturable.
 * ENERGIES.  tgnh_get_nonbonded_energy keeps its four slots; slot 0 is the direct-space sum while Ewald is on.  tgnh_get_ewald_energy
 * enqueues a one-work-group sum, synchronises `stream` and returns out[0] = E_rec, out[1] = E_self, out[2] = E_bg, out[3] = the
 * exclusion correction, kJ/mol, of the last want_energy call.  TGNH_ERR_STATE: Ewald is off; no tgnh_compute_nonbonded_force with
 * want_energy since the setting or the table was made, or since the per-cell buffers last grew; a host-only handle, buffers not
 * bound.  TGNH_ERR_ARG: out is NULL.  Setting or clearing Ewald closes tgnh_get_nonbonded_energy until the next want_energy call. */
typedef struct tgnh_ewald_desc {
    uint32_t struct_size;             /* sizeof(tgnh_ewald_desc); anything else: TGNH_ERR_ARG */
    int32_t kmax[3];                  /* reciprocal vectors n_d in [-kmax_d, kmax_d]; (0, 0, 0) is legal: no reciprocal part */
    double alpha;                     /* nm^-1 */
} tgnh_ewald_desc;
tgnh_status tgnh_set_nonbonded_ewald(tgnh_handle h, const tgnh_ewald_desc* d);          /* NULL: back to the reaction field */
tgnh_status tgnh_get_nonbonded_ewald(tgnh_handle h, tgnh_ewald_desc* out, int* num_kvectors);   /* struct_size 0 in *out: off */
tgnh_status tgnh_get_ewald_energy(tgnh_handle h, void* stream, double out[4]);          /* reciprocal, self, neutralising background, exclusion correction; synchronises */

/* PARTICLE-MESH EWALD: the same sum with the reciprocal part formed on a mesh (Essmann et al. 1995, OpenMM's `PME`), O(n + N log N)
 * in the slots n and the grid points N, for boxes the explicit sum cannot reach.  PME and the explicit sum are two forms of ONE
 * setting: each setter replaces whatever is in force, NULL to either goes back to the reaction field, and tgnh_set_nonbonded_force
 * drops either.  Everything under DIRECT SPACE, EXCLUSION CORRECTION, E_self and E_bg above holds unchanged with PME in force; only
 * RECIPROCAL SPACE is replaced by what follows.  With PME in force tgnh_get_nonbonded_ewald answers "off" (struct_size 0, M = 0),
 * tgnh_get_nonbonded_pme answers alpha and the grid, and tgnh_get_ewald_energy keeps its four slots, slot 0 being the mesh sum.  With
 * no PME setting nothing below is allocated or launched.  Nothing new is linked: the transform is the library's own.
 *
 * tgnh_set_nonbonded_pme(desc) follows tgnh_set_nonbonded_ewald point for point: it needs a CutoffPeriodic table in force
 * (TGNH_ERR_STATE), runs every check before any device work (a host-only handle answers alike), builds the setting aside and moves
 * it in whole, allocates and uploads everything the compute call will need (three grids of nx ny nz points: int64, complex fp64,
 * fp64; per axis a table of twiddle factors and one of moduli), and refuses with TGNH_ERR_STATE when the stream of the handle's last
 * tgnh_compute_nonbonded_force is capturing.  TGNH_ERR_ARG, with the reason in tgnh_last_error(): a struct_size that is not
 * sizeof(tgnh_pme_desc); an alpha that is not finite or <= 0; a grid component below 6, above 256, or with a prime factor other than
 * 2, 3, 5 (the text names the component).  TGNH_ERR_UNSUPPORTED: nx ny nz > 2^24.  The B-spline order is 5, a constant.  Formed at set
 * time on the host, per axis with N points:
 *   w^k      = (cos(2 pi k / N), -sin(2 pi k / N)), k < N, exact at the quarter turns: every twiddle factor of the transform is an
 *              entry of this table, so the transform kernels make no transcendental call
 *   |b(m)|^2 = (sum_j M(j) cos(2 pi m j / N))^2 + (sum_j M(j) sin(2 pi m j / N))^2, j = 0..3 in order, M = 1/24, 11/24, 11/24, 1/24,
 *              the cosines and sines being the table's entries at (m j) mod N; then, for m ascending, a modulus below 1e-7 is replaced
 *              by (|b(m - 1)|^2 + |b(m + 1)|^2) 0.5, indices mod N (OpenMM's rule: with order 5 the modulus vanishes at m = N / 2 for
 *              every even N)
 *   pi2 = pi pi     alpha2 = alpha alpha
 *
 * With PME on, tgnh_compute_nonbonded_force adds, behind the exclusion correction (fp64 in every precision, every operation rounded
 * on its own in the order written; the only library call is the exp of G):
 * WEIGHTS.  For slot i and an axis with N points and edge L:
 *   s = x / L;  s = s - floor(s);  t = s N;  i0 = (int)floor(t);  u = t - floor(t)
 *   th_0 = 1 - u, th_1 = u, th_2 = th_3 = th_4 = 0; then raise to order k for k = 3, 4:
 *     th_(k-1) = (u th_(k-2)) / (k - 1)
 *     th_(k-1-j) = ((u + j) th_(k-2-j) + ((k - j) - u) th_(k-1-j)) / (k - 1)      j = 1 .. k - 2
 *     th_0 = ((1 - u) th_0) / (k - 1)
 *   dth_0 = -th_0, dth_j = th_(j-1) - th_j (j = 1..4); then raise th to order 5 by the same three lines.
 *   Point j of the axis is (i0 + j) mod N (t can round up to N: the mod covers it).
 * SPREADING.  w = (thx_a thy_b) thz_c; grid point (a, b, c) of the slot receives llrint((q w) 281474976710656.0) (2^48) in an int64
 * grid Q[z][y][x] that the call clears first.  Integer adds commute: Q's bits depend on neither the order of arrival nor the order
 * of the slots.  A slot with q == 0 contributes nothing.  RANGE: a grid point holds up to 2^15 e of |q w|.
 * INFLUENCE FUNCTION.  For grid index m_d in [0, N_d): n_d = m_d if m_d <= N_d / 2 (integer division), else m_d - N_d;
 *   h_d = n_d / L_d;  m2 = (hx hx + hy hy) + hz hz;  V = (Lx Ly) Lz
 *   G = exp(-((pi2 m2) / alpha2)) / (((pi V) m2) ((|bx|^2 |by|^2) |bz|^2));  G(0, 0, 0) = 0
 * formed on the device from the box of the call: a box that changes between calls needs no reset.
 * TRANSFORMS.  F = DFT((double)Q 2^-48); phi = the real part of the unnormalised inverse DFT of G F.  A mixed-radix (4, 2, 3, 5)
 * Stockham transform of whole lines in LDS, five launches: x forward, y forward, z forward x G z inverse, y inverse, x inverse.  The
 * order of its sums depends on the grid alone; its rounding is not restated here (tests/test_pme.py measures how far an fp64 twin
 * built on another FFT is off an fp80 reference, and gates the device with that).
 * ENERGY.  E_rec = K sum over the z launch's work-groups of (1/2 sum_m G |F|^2), summed as the other energies' rows are.
 * FORCE.  g_d = sum over c (outermost), b, a (innermost) of (dth (in d) th th) phi, the product grouped as w is; slot i receives
 *   llrint((-(((K q_i) (N_d / L_d)) g_d)) 4294967296.0) once per component; a slot with charge 0 receives nothing.
 * PME does not conserve momentum exactly: the sum of the reciprocal forces falls with the grid spacing, it is not zero.
 * ORDER.  No floating-point atomic anywhere; the only atomics are the integer adds of the spreading.  The same positions, box and
 * tables give the same bits from a tiled, a TGNH_FLAG_GATHER and a DUALNH handle, asked once or twice, run eagerly or replayed from
 * a graph, and -- Q being a sum of integers and everything behind it a function of Q -- a permutation of the slots permutes the
 * force bits and leaves Q and phi alone.
 * LAUNCHES.  Behind the exclusion kernel: a memset of Q and seven kernels (spread, five transform launches, gather).  Capturable.
 * tgnh_get_pme_grids: host copies of the last call's Q and phi, [nz][ny][nx], either pointer may be NULL; synchronises `stream`.
 * TGNH_ERR_STATE: PME is off; no tgnh_compute_nonbonded_force has run since it was set (a call recorded into a capture has not run);
 * a host-only handle, buffers not bound. */
typedef struct tgnh_pme_desc {
    uint32_t struct_size;             /* sizeof(tgnh_pme_desc); anything else: TGNH_ERR_ARG */
    int32_t grid[3];                  /* nx, ny, nz: each in [6, 256] with prime factors 2, 3, 5 only; nx ny nz <= 2^24 */
    double alpha;                     /* nm^-1 */
} tgnh_pme_desc;
tgnh_status tgnh_set_nonbonded_pme(tgnh_handle h, const tgnh_pme_desc* d);              /* NULL: back to the reaction field */
tgnh_status tgnh_get_nonbonded_pme(tgnh_handle h, tgnh_pme_desc* out);                  /* struct_size 0 in *out: off */
tgnh_status tgnh_get_pme_grids(tgnh_handle h, void* stream, long long* charge, double* potential);   /* either may be NULL; [nz][ny][nx]; synchronises */

/* The call-outs of the reference's own testWater (platforms/reference/tests/TestReferenceDrudeTGNHIntegrator.cpp:111-166),
 * harness only: its force field -- NonbondedForce with reaction field, cutoff `cutoff` in a cubic box of edge `box`, +
 * DrudeForce + the M site's force spread over O, H1, H2, for slots laid out O, D, H1, H2, M per molecule -- written into
 * `force_out` in OpenMM's fixed-point layout, and OpenMM's CMMotionRemover on the bound velocities (one work-group, sized for
 * that test's 216 molecules and not for product use: tgnh_remove_cm_motion is the library's). */
tgnh_status tgnh_harness_water_force(tgnh_handle h, double box, double cutoff, void* force_out, void* stream);
tgnh_status tgnh_harness_remove_cm_motion(tgnh_handle h, void* stream);

/* Per-kernel launch statistics gathered with HIP events on `stream` while
 * enabled (bench.py's live roofline).  kernel: 0 scale+kick+drift, 1 kick+KE,
 * 2 rescale, 3 KE, 4 chain, 5 harness force, 6 other, 7 resident step.  on = 1: every kernel; on = 2 + k: kernel k only
 * (two event records per step instead of eight, for timing inside a throughput measurement); 0: off. */
tgnh_status tgnh_timing_enable(tgnh_handle h, int on);
tgnh_status tgnh_timing_read(tgnh_handle h, int kernel, double* total_ms, int64_t* launches);
/* Algorithmic HBM bytes of one launch of `kernel` (SURVEY.md 8d model: state arrays only). */
tgnh_status tgnh_algorithmic_bytes(tgnh_handle h, int kernel, double* bytes);

#ifdef __cplusplus
}
#endif
#endif
