// tgnh_lifecycle.cpp -- create (validate, decide path and launch policy, allocate, census), destroy, bound buffers, setters; the thread's last error
#include <memory>

#include "tgnh_host.h"
#ifndef TGNH_MEETING_MEM
#define TGNH_MEETING_MEM hipDeviceMallocFinegrained
#endif

static thread_local std::string g_err;
extern "C" const char* tgnh_last_error(void) { return g_err.c_str(); }
extern "C" int tgnh_abi_version(void) { return TGNH_ABI_VERSION; }

void tgnh_set_error(const std::string& msg) { g_err = msg; }

static tgnh_status validate_desc(const tgnh_desc* d, bool* long_chain) {
    if (d->struct_size != sizeof(tgnh_desc)) return fail(TGNH_ERR_ARG, "tgnh_desc size mismatch (ABI)");
    if (d->mode != TGNH_MODE_DUALNH && d->mode != TGNH_MODE_TGNH) return fail(TGNH_ERR_ARG, "bad mode");
    if (d->precision < TGNH_PREC_SINGLE || d->precision > TGNH_PREC_DOUBLE) return fail(TGNH_ERR_ARG, "bad precision");
    if (d->num_particles < 1 || d->num_pairs < 0 || !d->mass || (d->num_pairs && (!d->pair_drude || !d->pair_parent)))
        return fail(TGNH_ERR_ARG, "bad particle / pair arrays");
    if (d->padded_num_particles < d->num_particles) return fail(TGNH_ERR_ARG, "padded_num_particles < num_particles");
    if (d->num_constraints < 0) return fail(TGNH_ERR_ARG, "negative num_constraints");
    if (3LL * d->padded_num_particles > 2147483647LL)      // force[i + 2 paddedN] in 32-bit indices, here as in the reference's kernels (K :318-320)
        return fail(TGNH_ERR_UNSUPPORTED, "more than 715 827 882 padded particle slots: the index into the third force plane leaves 32 bits");
    if (d->num_nh_chains < 1 || d->drude_steps_per_real_step < 1) return fail(TGNH_ERR_ARG, "numNHChains and drudeStepsPerRealStep must be >= 1");
    if (d->mode == TGNH_MODE_TGNH && (d->num_groups < 1 || d->num_residues < 1 || !d->group || !d->resid))
        return fail(TGNH_ERR_ARG, "TGNH mode needs temperature groups and residues");
    if (!(d->max_drude_distance >= 0)) return fail(TGNH_ERR_ARG, "setMaxDrudeDistance: Distance cannot be negative");   // API :98-99 (NaN neither)
    if (d->flags & ~(uint32_t)(TGNH_FLAG_DEFER_SCALE | TGNH_FLAG_RESIDENT_STEP | TGNH_FLAG_WAVE_TILES | TGNH_FLAG_TRUST_STATE_CHANGED | TGNH_FLAG_GATHER))
        return fail(TGNH_ERR_ARG, "unknown bits in tgnh_desc.flags (a newer header than this library?)");
    if (d->mode == TGNH_MODE_DUALNH && d->num_pairs == 0)   // Ref :181 reads pairParticles[0]; its chain divides by the Drude thermostat mass 0
        return fail(TGNH_ERR_UNSUPPORTED, "dualNH mode needs at least one Drude pair (the Reference platform does too)");
    if (!(d->step_size > 0) || !std::isfinite(d->step_size)) return fail(TGNH_ERR_ARG, "step size must be positive");
    *long_chain = false;
    {   // the chain kernel keeps chains longer than 4 links (16 in TGNH mode: chain_long_kernel) in a 2048-double LDS scratch; what
        // does not fit runs a thermostat per thread with its links in global memory (gather_chain_kernel, TGNH mode)
        const long need = d->mode == TGNH_MODE_TGNH ? (long)(d->num_groups + 2) * (4L * d->num_nh_chains + 1)
                                                    : 4L * (2L * d->num_nh_chains + 4);
        if (d->num_nh_chains > (d->mode == TGNH_MODE_TGNH ? 16 : 4) && need > 2048) {
            if (d->mode != TGNH_MODE_TGNH) return fail(TGNH_ERR_UNSUPPORTED, "numNHChains too large for the on-device chain");
            *long_chain = true;
        }
    }
    return TGNH_OK;
}

// which path steps this topology, and how its launches are shaped
static tgnh_status decide_policy(tgnh_context* c, const tgnh_desc* d, bool long_chain) {
    if (c->gather.generic) {
        // The gather path steps in the reference's own pass structure, velocities never lagging: the flags that change the
        // structure are dropped (all of them leave the trajectory what it is; tgnh_flush has nothing to do, state setters
        // between steps are allowed as without TGNH_FLAG_DEFER_SCALE)
        c->d.flags &= ~(TGNH_FLAG_DEFER_SCALE | TGNH_FLAG_RESIDENT_STEP | TGNH_FLAG_TRUST_STATE_CHANGED | TGNH_FLAG_WAVE_TILES);
        c->gather.chain = c->d.mode == TGNH_MODE_TGNH && (c->thermo.L.NT > MAX_GROUPS + 2 || long_chain);
    }
    // KE passes and the one-launch step over wave tiles: register bins (G <= 8), and tiles that fill their wavefront -- a wave
    // tile ends where a molecule does, so 35-slot cations leave 45 of 64 lanes busy and the 512-slot tiles, cut the same way but
    // eight times as long, win (ionic liquid 100 k: 42.0 k steps/s on the tile kernels, 40.3 k on wave tiles; 60-slot water
    // tiles: 94 % full)
    c->cfg.wave_ke = !c->gather.generic && !c->topo.wave_tile.empty() && c->cfg.gb != 0 &&
                 ((d->flags & TGNH_FLAG_WAVE_TILES) || (double)d->num_particles >= 0.9 * WAVE_SLOTS * (double)c->topo.num_wtiles);
#ifdef TGNH_TUNING
    if (const char* e = getenv("TGNH_WAVE_KE")) c->cfg.wave_ke = c->cfg.wave_ke && e[0] != '0';
#endif
    {   // s^2 KE is the exact post-rescale KE only if no molecule spans two temperature groups: v_rel = v - v_com of such a
        // molecule is scaled by two different factors, which moves its centre of mass (K :260-300)
        bool inside = true;
        if (com_thermostat_on(*d)) {
            std::vector<int> g0(d->num_residues, -1);      // (by particle, not by (first, count): a residue may come in several runs)
            for (int i = 0; i < d->num_particles && inside; i++) {
                if (c->topo.mass[i] == 0.0) continue;
                int& g = g0[c->topo.resid[i]];
                if (g == -1) g = c->topo.group[i];
                else if (g != c->topo.group[i]) inside = false;
            }
        }
        if ((c->d.flags & TGNH_FLAG_DEFER_SCALE) && !inside) return fail(TGNH_ERR_UNSUPPORTED, "DEFER_SCALE needs every molecule inside one temperature group");
        // TRUST_STATE_CHANGED (the reference's pass structure without the begin half's KE pass) asks the same of the topology;
        // where it does not hold the flag is ignored -- the handle recomputes, as without it (tgnh_get_pending_state bit 9 never shows)
        c->cfg.carry_ok = (c->d.flags & TGNH_FLAG_TRUST_STATE_CHANGED) && !(c->d.flags & TGNH_FLAG_DEFER_SCALE) && inside;
    }
    c->cfg.grid = GRID_CAP;                       // partials are sized for the largest grid
#ifdef TGNH_TUNING       // environment knobs exist in tuning builds only (tools/build_variant.py -DTGNH_TUNING)
    if (const char* e = getenv("TGNH_GRID")) { int g = atoi(e); if (g >= 1) c->cfg.grid_override = std::min(g, GRID_CAP); }
#endif
    {   // One-link chains run inside the rescale launch: one wavefront per work-group computes the factors while
        // the other three have their tile loads in flight, so the chain (~3.5 us) costs the launch nothing, and
        // the chain launch that remains only sums the partial rows (profiles/r01_tuning_sweep.log: +7 % steps/s
        // at 625 k slots, +1.5 % at 5 M).
        bool want = true;
        // The partial rows are summed in that prologue too (no sum launch) up to 2 M slots: beyond, the launches are
        // bandwidth-bound, the gain shrinks to 0.7 % and the row read would only lengthen the dominant launch
        c->cfg.inline_sum_all = d->num_particles < 2000000;
#ifdef TGNH_TUNING
        if (const char* e = getenv("TGNH_INLINE_CHAIN")) want = e[0] != '0';
        if (const char* e4 = getenv("TGNH_INLINE_SUM_ROWS")) c->cfg.inline_sum_rows = atoi(e4);   // 0 = never
        if (const char* e5 = getenv("TGNH_INLINE_SUM_ALL")) c->cfg.inline_sum_all = e5[0] != '0';
        if (const char* e3 = getenv("TGNH_ALTERNATE_SWEEPS")) c->cfg.alternate_sweeps = e3[0] != '0';
#endif
        // dualNH qualifies too: with useDrudeNHChains its real and Drude chains are independent (Chain1Map), without
        // them coupled through one shuffle per sub-step (chain1q_run)
        // Chains of 2-4 links too, but in instantiations of their own that hold two work-groups per compute unit where the
        // one-link kernels hold three (the links' registers): taken below 2.5 M slots.  Beyond, the streaming launches are
        // bandwidth-bound and keep their occupancy -- chain_kernel's 18 us cost less.  (The limit was 1 M slots while a launch's
        // chain wavefront ran the real thermostats and the Drude thermostat one after the other; with both in one pass,
        // chain_both_fast, three links inside the launches read +16 % at 625 k slots, +7 % at 1.25 M, +3..6 % at 2 M and
        // -4 % / +1 % (one launch per step / deferred) at 5 M: tools/micro/inline_multi_threshold.py,
        // profiles/r04_inline_multi_threshold.txt)
        int inline_multi_max = 2500000;
#ifdef TGNH_TUNING
        if (const char* e6 = getenv("TGNH_INLINE_MULTI_MAX")) inline_multi_max = atoi(e6);
#endif
        c->cfg.inline_chain = want && !c->gather.generic && (c->thermo.L.C == 1 || (c->thermo.L.C <= 4 && d->num_particles < inline_multi_max));
        if (c->thermo.L.total > 256 && c->thermo.L.C > 1) c->cfg.inline_chain = c->cfg.inline_chain && false;     // (wstep_kernel parks the block in 256 doubles)
    }
    return TGNH_OK;
}

static tgnh_status allocate(tgnh_context* c) {
    const size_t NT = c->thermo.L.NT;
    HIP_OK(c->thermo.d_partials.alloc((size_t)(c->cfg.grid + c->topo.num_big) * NT, true));
    HIP_OK(c->thermo.d_state.alloc(c->thermo.L.total));
    HIP_OK(c->thermo.d_stage.alloc(c->thermo.L.total));
    HIP_OK(c->status.d_word.alloc(1, true));
    HIP_OK(c->status.h_seen.alloc_pinned(1));
    *c->status.h_seen = 0;
    if (c->gather.chain && c->thermo.L.C > 4) HIP_OK(c->gather.d_scratch.alloc(NT * (4 * c->thermo.L.C + 1)));
    HIP_OK(c->thermo.d_scalar.alloc(1 + PLAIN_KE_PARTS));
    HIP_OK(c->meet.d_sync.alloc(4, true));
    const bool resident = (c->d.flags & TGNH_FLAG_RESIDENT_STEP) != 0;
    if (c->cfg.wave_ke || resident)                                       // the tagged rows of wke_kernel's tail sum, or of step_kernel
        HIP_OK(c->meet.d_rows.alloc(2 * (size_t)GRID_CAP * CHAIN_INLINE_SUM_NT, true, TGNH_MEETING_MEM));
    if (!resident) return TGNH_OK;
    // step_kernel's meeting place: the work-groups' tagged rows, and a private one-rank mailbox that carries the
    // sums from work-group 0 to all the others when no sharded exchange is attached.  Both stay on this device:
    // fine-grained memory (a flag stored by one work-group is seen by a polling one on another XCD after 0.37-0.39 us,
    // uncached memory takes 0.58-0.63: tools/micro/hop_probe.hip); the mailboxes peers store into are uncached
    HIP_OK(c->meet.self_box.alloc(XCHG_MAILBOX_BYTES(1) / sizeof(unsigned long long), true, TGNH_MEETING_MEM));
    HIP_OK(c->meet.d_self_misc.alloc(4, true));                             // [0] seq, [1] dead latch, [2] peers[0]
    unsigned long long* const box = c->meet.self_box;
    HIP_OK(hipMemcpy(c->meet.d_self_misc + 2, &box, sizeof(box), hipMemcpyHostToDevice));
    c->meet.self_x = XchgArgs{};
    c->meet.self_x.on = 1; c->meet.self_x.world = 1; c->meet.self_x.rank = 0;
    c->meet.self_x.peers = reinterpret_cast<unsigned long long* const*>(c->meet.d_self_misc + 2);
    c->meet.self_x.mine = c->meet.self_box;
    c->meet.self_x.seq = c->meet.d_self_misc;
    c->meet.self_x.dead = reinterpret_cast<unsigned int*>(c->meet.d_self_misc + 1);
    c->meet.self_x.status = c->status.d_word;
    return TGNH_OK;
}

// How many work-groups per compute unit are resident TOGETHER?  The occupancy API's answer (at most 8) is checked by a census
// launch (every work-group checks in and waits for all the others, bounded); one fewer per unit is tried until a grid passes.
template <typename Launch> static tgnh_status census(tgnh_context* c, int per_cu_max, Launch&& launch, int* found) {
    for (int per_cu = std::min(per_cu_max, 8); per_cu >= 1 && !*found; per_cu--) {
        TileArgs a{};
        a.census = 1; a.sync = c->meet.d_sync;
        HIP_OK(hipMemset(c->meet.d_sync + 2, 0, 2 * sizeof(unsigned int)));
        const int grid = std::min(per_cu * c->cfg.num_cus, GRID_CAP);
        HIP_OK(launch(a, grid));
        unsigned int res[2] = {0, 1};
        HIP_OK(hipMemcpy(res, c->meet.d_sync + 2, sizeof(res), hipMemcpyDeviceToHost));
        if (res[0] == (unsigned)grid && res[1] == 0) *found = per_cu;
    }
    return TGNH_OK;
}

// step_kernel's and wstep_kernel's resident counts.  0 = no grid passed: the handle steps the DEFER_SCALE way.
static tgnh_status resident_census(tgnh_context* c) {
    if (!(c->d.flags & TGNH_FLAG_RESIDENT_STEP) || c->cfg.gb == 0 || !c->cfg.inline_chain || c->thermo.L.NT > CHAIN_INLINE_SUM_NT) return TGNH_OK;
    // (the kind with the largest footprint this handle will launch: a whole deferred step, or the plain begin half)
    const int kind = pass_kind(c->d);
    const size_t lds = tile_lds_bytes(c->d.precision, step_kind_ops2(kind), true, true);
    // (step_kernel runs one-link chains only; longer ones have wstep_kernel below, or the launches)
    tgnh_status rc = census(c, c->thermo.L.C == 1 ? step_blocks_per_cu(c->d.precision, c->cfg.gb, kind, lds) : 0,
                            [&](const TileArgs& a, int grid) { return launch_step(c->d.precision, c->cfg.gb, kind, a, grid, lds, (hipStream_t)0); },
                            &c->cfg.resident_per_cu);
    if (rc) return rc;
    // the same count for wstep_kernel, which runs the whole deferred step when the topology has wave tiles
    const bool multi = c->thermo.L.C > 1;
    bool want_w = c->cfg.wave_ke && (c->d.flags & TGNH_FLAG_DEFER_SCALE) && (c->cfg.resident_per_cu > 0 || multi);
    // dualNH's coupled chain (useDrudeNHChains = false) of 2-4 links: wstep_kernel has no room for its fast form beside its
    // 228 registers (chainN_run<false>), the rescale launches have -- and every kernel of every rank must run the SAME
    // arithmetic (replicated chains stay bit-identical): such a handle steps the DEFER_SCALE way, chain inside the launch
    if (c->d.mode == TGNH_MODE_DUALNH && !c->thermo.L.use_drude_chains && multi) want_w = false;
#ifdef TGNH_TUNING
    if (const char* e = getenv("TGNH_WSTEP")) want_w = want_w && e[0] != '0';
#endif
    return census(c, want_w ? wstep_blocks_per_cu(c->d.precision, c->cfg.gb, multi) : 0,
                  [&](const TileArgs& a, int grid) { return launch_wstep(c->d.precision, c->cfg.gb, multi, a, grid, (hipStream_t)0); },
                  &c->cfg.wresident_per_cu);
}

// The one-launch step's velocity planes (tgnh_context.h VelPlanes), for a handle that can take them: it steps with wstep_kernel
// (a whole deferred step over wave tiles: the census above found a grid), every wave tile is patterned and every slot's mass is
// its pattern entry's -- then 1/m is a function of a lane's place in the pattern and the kernel needs no w per slot.  Allocated
// here and never later (an allocation inside somebody's stream capture would fail it): 3 x stride x sizeof(mixed), the stride the
// box's massive slots with every wave tile's segment padded to a 128-byte line (tgnh_topology.cpp) -- 96 MB for a water box of
// 5 M slots in mixed precision.  TGNH_VELOCITY_PLANES=0 in the environment keeps a handle on velm (both forms from one build).
static tgnh_status allocate_velocity_planes(tgnh_context* c) {
    if (const char* e = getenv("TGNH_VELOCITY_PLANES")) if (e[0] == '0') return TGNH_OK;
    if (!(c->d.flags & TGNH_FLAG_DEFER_SCALE) || c->cfg.wresident_per_cu <= 0 || !c->topo.wpat_all_uniform || c->topo.wtile_base.empty()) return TGNH_OK;
    // Single precision stays on velm: there the two kernels do not give the same bits (tgnh_wave_kernels.h, wstep_fn_gb)
    if (c->d.precision == TGNH_PREC_SINGLE) return TGNH_OK;
    // (the census counted work-groups of wstep_kernel: wstep_planes_kernel meets on the same grid, so it must hold as many per compute unit)
    if (wstep_blocks_per_cu(c->d.precision, c->cfg.gb, c->thermo.L.C > 1, true) < c->cfg.wresident_per_cu) return TGNH_OK;
    const bool single = c->d.precision == TGNH_PREC_SINGLE;
    const size_t word = single ? sizeof(float) : sizeof(double), n = c->topo.wpat_mass.size();
    // what velm's w holds for a slot of mass m: 1 / m in fp64, rounded to velm's type; 0 for a massless slot
    std::vector<double> inv(n);
    for (size_t k = 0; k < n; k++) inv[k] = c->topo.wpat_mass[k] == 0.0 ? 0.0 : 1.0 / c->topo.wpat_mass[k];
    std::vector<float> inv_f(inv.begin(), inv.end());
    HIP_OK(c->vp.d_invm.upload(reinterpret_cast<const unsigned char*>(single ? (const void*)inv_f.data() : (const void*)inv.data()), n * word));
    HIP_OK(c->vp.d_mismatch.alloc(1, true));
    // the planes hold the massive slots only: a tile's segment at wtile_base[tile], a lane's word wpat_off[pattern][lane] into it
    c->vp.stride = (int)c->topo.wtile_base.back();
    HIP_OK(c->vp.d_base.upload(c->topo.wtile_base));
    HIP_OK(c->vp.d_off.upload(c->topo.wpat_off));
    HIP_OK(c->vp.d_planes.alloc(3 * (size_t)std::max(c->vp.stride, 1) * word, true));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_create(const tgnh_desc* d, tgnh_handle* out) {
    if (!d || !out) return fail(TGNH_ERR_ARG, "null argument");
    bool long_chain = false;
    tgnh_status rc = validate_desc(d, &long_chain); if (rc) return rc;
    // device == -1: host-only handle for the host logic (topology, tiles, dof); every launch on it fails
    const bool host_only = d->device == -1;
    if (!host_only) {
        int ndev = 0;
        HIP_OK(hipGetDeviceCount(&ndev));
        if (d->device < 0 || d->device >= ndev) return fail(TGNH_ERR_HIP, "no such HIP device (the HIP path needs an MI355X; there is no CPU fallback)");
        HIP_OK(hipSetDevice(d->device));
    }

    std::unique_ptr<tgnh_context> owner(new tgnh_context());    // (released with the device just set current, like tgnh_destroy)
    tgnh_context* c = owner.get();
    c->host_only = host_only;
    c->d = *d;
    c->device = d->device;
    set_bath_temperatures(c, d->temperature, d->drude_temperature);
    make_layout(c);
    c->cfg.gb = c->thermo.L.G <= 1 ? 1 : (c->thermo.L.G <= 4 ? 4 : (c->thermo.L.G <= 8 ? 8 : 0));   // 0: KE bins in LDS
    if (long_chain) { c->gather.generic = true; c->gather.reason = "a chain too long for the LDS-resident form"; }
    else if (d->flags & TGNH_FLAG_GATHER) { c->gather.generic = true; c->gather.reason = "asked for (TGNH_FLAG_GATHER)"; }
    if (!host_only) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d->device) == hipSuccess && prop.multiProcessorCount > 0) c->cfg.num_cus = prop.multiProcessorCount;
    }
    rc = build_topology(c, d); if (rc) return rc;
    rc = decide_policy(c, d, long_chain); if (rc) return rc;
    local_dof_terms(c);
    c->thermo.global_terms = c->thermo.local_terms;
    // constraint arrays are only needed during create
    c->d.mass = nullptr; c->d.pair_drude = c->d.pair_parent = c->d.group = c->d.resid = nullptr;
    c->d.constraint_i = c->d.constraint_j = nullptr;

    if (!host_only) {
        rc = allocate(c); if (rc) return rc;
        rc = resident_census(c); if (rc) return rc;
        rc = allocate_velocity_planes(c); if (rc) return rc;
    }
    rc = finalize_thermostat(c); if (rc) return rc;
    *out = owner.release();
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_destroy(tgnh_handle h) {
    CHECK_H(h);
    if (h->xchg.rccl_comm) (void)tgnh_rccl_shutdown(h);
    if (!h->host_only) (void)hipSetDevice(h->device);
    delete h;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_bind_buffers(tgnh_handle h, void* posq, void* posq_correction, void* velm,
                                         const void* force, void* pos_delta) {
    CHECK_H(h);
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle (device -1): no GPU work can be launched on it");
    if (!posq || !velm || !force) return fail(TGNH_ERR_ARG, "posq, velm and force are required");
    if (h->d.precision == TGNH_PREC_MIXED && !posq_correction) return fail(TGNH_ERR_ARG, "mixed precision needs posqCorrection");
    if ((h->owed.kick_pending || h->owed.end_pending) && (velm != h->bound.velm || force != h->bound.force))
        return fail(TGNH_ERR_STATE, "tgnh_bind_buffers: velm / force may not be rebound while a deferred half kick is pending (tgnh_flush first)");
    if (posq == h->bound.posq && posq_correction == h->bound.posq_corr && velm == h->bound.velm && force == h->bound.force && pos_delta == h->bound.pos_delta)
        return TGNH_OK;                                   // (the glue binds at every step: the same arrays, nothing to do)
    {   // Every kernel indexes these arrays by slot without a bound of its own: an allocation shorter than N slots (or 3 planes
        // of `padded`) would be a write off its end on the device.  Where the runtime knows the allocation a pointer lies in,
        // what is left of it behind the pointer must cover what the launches touch (a sub-allocation of a caching allocator
        // passes with its block's size: a lower bound, but the gross cases -- a float4 array bound as double4, N for padded --
        // are caught here, on the host, with a message).
        HIP_OK(hipSetDevice(h->device));
        const size_t N = (size_t)h->d.num_particles, P = (size_t)h->d.padded_num_particles;
        const size_t r4 = h->d.precision == TGNH_PREC_DOUBLE ? 32 : 16, m4 = h->d.precision == TGNH_PREC_SINGLE ? 16 : 32;
        struct { const void* p; size_t need; const char* name; } bufs[] = {
            {posq, N * r4, "posq"}, {posq_correction, N * 16, "posqCorrection"}, {velm, N * m4, "velm"},
            {force, 3 * P * sizeof(long long), "force"}, {pos_delta, N * m4, "posDelta"}};
        for (const auto& b : bufs) {
            if (!b.p) continue;
            hipDeviceptr_t base = nullptr; size_t size = 0;
            if (hipMemGetAddressRange(&base, &size, const_cast<void*>(b.p)) != hipSuccess) { (void)hipGetLastError(); continue; }   // not known to the runtime (mapped by other means): the caller's word is taken
            const size_t left = size - (size_t)(static_cast<const char*>(b.p) - static_cast<const char*>(base));
            if (left < b.need)
                return fail(TGNH_ERR_ARG, std::string("tgnh_bind_buffers: ") + b.name + " has " + std::to_string(left) + " bytes behind the pointer, the launches touch " + std::to_string(b.need));
        }
    }
    h->owed.ke_carry = false;                                  // (other buffers: nothing computed from the old ones carries over)
    if (velm != h->bound.velm) {
        // Velocity planes live here: the call comes between tgnh_step_begin and tgnh_step_end (nothing is pending, see above).  The
        // array that goes gets the velocities back first, as a caller who copies it expects; the new one's w is checked anew, and
        // steps recorded on the old one no longer pin the handle (their graph holds the old pointer).
        tgnh_status rc = velm_current(h, h->vp.stream); if (rc) return rc;
        h->vp.verdict = 0; h->vp.pinned = false; h->vp.streak = 0;
    }
    if (posq != h->bound.posq || posq_correction != h->bound.posq_corr) h->snap.valid = false;      // (tgnh_restore_positions: its snapshot is of the old arrays)
    h->bound.posq = posq; h->bound.posq_corr = posq_correction; h->bound.velm = velm; h->bound.force = force; h->bound.pos_delta = pos_delta;
    return TGNH_OK;
}

tgnh_status deferred_guard(tgnh_handle h, const char* what) {
    if (h->owed.first_half_done || h->owed.end_pending)
        return fail(TGNH_ERR_STATE, std::string(what) + ": not allowed between steps with TGNH_FLAG_DEFER_SCALE (the next thermostat half step has already run)");
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_step_size(tgnh_handle h, double dt) {
    CHECK_H(h);
    if (!(dt > 0) || !std::isfinite(dt)) return fail(TGNH_ERR_ARG, "step size must be positive");
    if (dt != h->d.step_size) { tgnh_status rc = deferred_guard(h, "tgnh_set_step_size"); if (rc) return rc; }
    h->d.step_size = dt;
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_set_drude_steps_per_real_step(tgnh_handle h, int n) {
    CHECK_H(h);
    if (n < 1) return fail(TGNH_ERR_ARG, "drudeStepsPerRealStep must be >= 1");
    if (n != h->d.drude_steps_per_real_step) { tgnh_status rc = deferred_guard(h, "tgnh_set_drude_steps_per_real_step"); if (rc) return rc; }
    h->d.drude_steps_per_real_step = n;
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_set_max_drude_distance(tgnh_handle h, double dist) {
    CHECK_H(h);
    if (!(dist >= 0)) return fail(TGNH_ERR_ARG, "setMaxDrudeDistance: Distance cannot be negative");   // API :98-99 (NaN neither)
    h->d.max_drude_distance = dist;
    return TGNH_OK;
}

// Both baths of a live handle.  Everything the temperatures decide is formed again by what tgnh_create ran
// (set_bath_temperatures, thermostat_targets): the handle holds what one created at these temperatures holds; of the block only
// N kT and the thermostat masses go to the device -- eta, etaDot, etaDotDot are the run's.
extern "C" tgnh_status tgnh_set_temperatures(tgnh_handle h, double temperature, double drude_temperature, void* stream) {
    CHECK_H(h);
    tgnh_status rc = check_temperatures(temperature, drude_temperature); if (rc) return rc;
    rc = deferred_guard(h, "tgnh_set_temperatures"); if (rc) return rc;
    const ChainLayout& L = h->thermo.L;
    hipStream_t s = (hipStream_t)stream;
    rc = entry(h, false); if (rc) return rc;
    if (!h->host_only) { rc = materialize_chain(h, s); if (rc) return rc; }   // (a chain still owed runs at the temperature it was owed at; a staged block is committed)
    h->owed.ke_carry = false;
    set_bath_temperatures(h, temperature, drude_temperature);
    std::vector<double> st(L.total, 0.0);
    thermostat_targets(h, st);
    const int sections[2][2] = {{L.off_etaMass, L.len_etaMass}, {L.off_nkbt, L.NT}};
    for (const auto& sec : sections) std::copy(st.begin() + sec[0], st.begin() + sec[0] + sec[1], h->thermo.h_state.begin() + sec[0]);
    if (h->host_only) return TGNH_OK;
    for (const auto& sec : sections) {                           // both copies, as tgnh_set_thermostat_state
        HIP_OK(hipMemcpyAsync(h->thermo.d_state + sec[0], st.data() + sec[0], sizeof(double) * sec[1], hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(h->thermo.d_stage + sec[0], st.data() + sec[0], sizeof(double) * sec[1], hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipStreamSynchronize(s));                             // (st is pageable and about to go)
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_local_dof_terms(tgnh_handle h, double* terms, int* count) {
    CHECK_H(h);
    if (count) *count = h->thermo.L.NT;
    if (terms) std::copy(h->thermo.local_terms.begin(), h->thermo.local_terms.end(), terms);
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_set_global_dof_terms(tgnh_handle h, const double* terms, int count) {
    CHECK_H(h);
    if (!terms || count != h->thermo.L.NT) return fail(TGNH_ERR_ARG, "dof term count mismatch");
    if (h->run.step_count != 0) return fail(TGNH_ERR_STATE, "global dof must be set before the first step");
    if (!h->host_only) HIP_OK(hipSetDevice(h->device));
    h->thermo.global_terms.assign(terms, terms + count);
    return finalize_thermostat(h);
}
