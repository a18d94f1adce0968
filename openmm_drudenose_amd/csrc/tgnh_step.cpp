// tgnh_step.cpp -- step orchestration (A11): device-reported failures, the launch decisions by name, launch sizing, run_tile / run_gather / run_chain / run_resident, tgnh_step_*, flush, clock
#include "tgnh_host.h"

// ---------------------------------------------------------------------------
// device-reported failures
// ---------------------------------------------------------------------------
constexpr int64_t STATUS_POLL_EVERY = 64;

// Called wherever the status word has reached the host.  bit 2: a mailbox exchange timed out -- from then on the
// kinetic-energy sums are incomplete and the ranks' thermostats diverge; bit 0 in dualNH mode: the Reference platform
// throws (Ref :311-312).  Both make every later step / query fail (entry()).  bit 1 (the harness SHAKE did not
// converge) is reported by tgnh_get_status_flags only: OpenMM's own constraint kernels do not throw either.
void note_status(tgnh_handle h, uint32_t flags) {
    if (h->status.failed_code) return;
    // bit 3 first: when step_kernel's work-group 0 gives up on a row it sets bit 3 and withholds the sums, and every other
    // work-group then runs into its own time-out (bit 2) -- a residency problem, not a link fault
    if (flags & 8u) {
        h->status.failed_code = TGNH_ERR_STATE;
        h->status.failed = "resident step (noticed at step " + std::to_string((long long)h->run.step_count) + "): the launch's work-groups did "
                    "not all become resident within the time limit (TGNH_FLAG_RESIDENT_STEP needs the device to itself)";
        if (flags & 4u) h->status.failed += "; the waiting work-groups timed out in turn (status bits 2 and 3)";
    } else if (flags & 16u) {
        h->status.failed_code = TGNH_ERR_STATE;
        h->status.failed = "kinetic-energy pass (noticed at step " + std::to_string((long long)h->run.step_count) + "): work-group 0 did not "
                    "receive every work-group's row of sums within the time limit (the sums were left as NaN: nothing integrated "
                    "on with a partial sum); the device is shared with something that keeps this launch's work-groups from running "
                    "-- or a chain was handed a NaN kinetic energy: with an all-reduce attached, the rank on which that happened";
    } else if (flags & 4u) {
        h->status.failed_code = TGNH_ERR_STATE;
        h->status.failed = "mailbox exchange timed out (noticed at step " + std::to_string((long long)h->run.step_count) +
                    "): a peer did not send its kinetic-energy sums; the run cannot continue";
    } else if ((flags & 1u) && h->d.mode == TGNH_MODE_DUALNH) {
        h->status.failed_code = TGNH_ERR_HARDWALL;
        h->status.failed = "Drude particle moved too far beyond hard wall constraint";        // Ref :311-312
    }
}

tgnh_status finish_query(tgnh_handle h, hipStream_t s) {
    HIP_OK(hipMemcpyAsync(h->status.h_seen, h->status.d_word, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    note_status(h, *h->status.h_seen);       // what was just read may come from a failed exchange: say so now
    if (h->status.failed_code) return fail(h->status.failed_code, h->status.failed);
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return s != nullptr && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

static tgnh_status need_buffers(tgnh_handle h) {
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle (device -1): no GPU work can be launched on it");
    if (!h->bound.velm) return fail(TGNH_ERR_STATE, "tgnh_bind_buffers has not been called");
    return TGNH_OK;
}

// ---- what the handle's configuration decides, each fact once ----
// The next rescale launch sums `rows` partial rows in its prologue and runs the chain itself: nothing is launched between a KE
// pass and it.  Asked by both who-sums-the-rows decisions: the KE launch's tail sum (ke_pass_prologue) and run_chain.
static bool rescale_sums_rows(tgnh_handle h, int rows) {
    return h->cfg.inline_chain && !h->xchg.on && !h->xchg.allreduce && h->thermo.L.NT <= CHAIN_INLINE_SUM_NT &&
           (rows + h->topo.num_big <= h->cfg.inline_sum_rows || h->cfg.inline_sum_all);
}
// After this end half the stored velocities have the bins ke_post, until somebody writes velocities (unsharded only: a rank that
// recomputes while its peers carry over would enter a collective alone)
static bool ke_carries(tgnh_handle h) { return h->cfg.carry_ok && !h->xchg.allreduce && !h->xchg.on; }
// molecules longer than a tile whose centre-of-mass velocities the rescale launches read from a table (run_big_com)
bool big_com_on(tgnh_handle h) { return h->topo.num_big && com_thermostat_on(h->d); }
tgnh_status allreduce_doubles(tgnh_handle h, double* device_ptr, int count, hipStream_t s) {
    if (h->xchg.allreduce && h->xchg.allreduce(device_ptr, count, (void*)s, h->xchg.allreduce_user) != 0)
        return fail(TGNH_ERR_HIP, "all-reduce hook failed");
    return TGNH_OK;
}
tgnh_status allreduce_hook(tgnh_handle h, hipStream_t s) { return allreduce_doubles(h, h->thermo.d_state + h->thermo.L.off_ke_red, h->thermo.L.NT, s); }
static tgnh_status timed_chain(tgnh_handle h, const ChainArgs& a, hipStream_t s) { Timed t(h, s, KID_CHAIN); HIP_OK(launch_chain(a, s)); return TGNH_OK; }

// the fields TileArgs and GatherArgs share by name
template <typename Args> static Args common_args(tgnh_handle h, const double* scale) {
    Args a{};
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr; a.velm = h->bound.velm;
    a.force = reinterpret_cast<const long long*>(h->bound.force); a.pos_delta = h->bound.pos_delta;
    a.scale = scale ? scale : h->thermo.d_state + h->thermo.L.off_scale;
    a.partials = h->thermo.d_partials; a.status = h->status.d_word;
    a.padded = h->d.padded_num_particles;
    a.use_com = com_thermostat_on(h->d) ? 1 : 0;
    a.hardwall = h->d.max_drude_distance > 0 ? 1 : 0;                         // Ref :299, Cu :372
    a.dt = h->d.step_size; a.max_dist = h->d.max_drude_distance;
    a.hw_scale = std::sqrt(h->d.kB * h->d.drude_temperature);                 // Ref :300, Cu :299
    return a;
}

static TileArgs tile_args(tgnh_handle h, const double* scale) {
    TileArgs a = common_args<TileArgs>(h, scale);
    a.meta = h->topo.d_meta; a.tile_start = h->topo.d_tile_start; a.tile_res = h->topo.d_tile_res; a.res_table = h->topo.d_res_table;
    a.big_com = h->topo.d_big_com;
    a.num_tiles = h->topo.num_tiles; a.num_groups = h->thermo.L.G;
    a.reverse = h->run.sweep_reverse;
    a.wave_tile = h->topo.d_wave_tile; a.wmeta = h->topo.d_wmeta; a.num_wtiles = h->topo.num_wtiles;
    a.tile_pat = h->topo.d_tile_pat; a.pattern = h->topo.d_pattern; a.wpattern = h->topo.d_wpattern;
    return a;
}

// persistent grid = the work-groups of this instantiation that are resident at once (occupancy x CUs), so every
// work-group walks the same number of tiles (+-1) and there is no partial last wave of work-groups
static int grid_for(tgnh_handle h, int ops, bool hardwall, size_t lds) {
    if (h->cfg.grid_override > 0) return std::min(h->topo.num_tiles, h->cfg.grid_override);
    const int key = ops | (hardwall ? 1 << 16 : 0);
    auto it = h->cfg.grid_cache.find(key);
    if (it != h->cfg.grid_cache.end()) return it->second;
    int per_cu = tile_blocks_per_cu(h->d.precision, ops, h->cfg.gb, lds, (ops & OP_SCALE) && h->cfg.inline_chain && h->thermo.L.C > 1);
    if (per_cu < 1) per_cu = 2;
    int g = std::min(std::min(h->topo.num_tiles, per_cu * h->cfg.num_cus), GRID_CAP);
    if (g < 1) g = 1;
    h->cfg.grid_cache[key] = g;
    return g;
}

// wke_kernel: the resident work-groups, at most one per four wavefront tiles
static int wave_grid_for(tgnh_handle h, int ops) {
    const int nw = h->topo.num_wtiles, need = (nw + TBLOCK / 64 - 1) / (TBLOCK / 64);
    if (h->cfg.grid_override > 0) return std::max(1, std::min(need, h->cfg.grid_override));
    const int key = ops | (1 << 17);
    auto it = h->cfg.grid_cache.find(key);
    if (it != h->cfg.grid_cache.end()) return it->second;
    int per_cu = wke_blocks_per_cu(h->d.precision, ops, h->cfg.gb);
    if (per_cu < 1) per_cu = 2;
#ifdef TGNH_TUNING
    if (const char* e = getenv("TGNH_WKE_PER_CU")) { int v = atoi(e); if (v >= 1) per_cu = std::min(per_cu, v); }
#endif
    int g = std::max(1, std::min(std::min(need, per_cu * h->cfg.num_cus), GRID_CAP));
    h->cfg.grid_cache[key] = g;
    return g;
}

static tgnh_status commit_stage(tgnh_handle h, hipStream_t s);

// words of the tagged-row area (TileArgs::rows) and what a launch of `grid` work-groups with NT thermostats writes there
// (row_word in tgnh_xchg_device.h: rows in blocks of 64, word-major inside a block, two words per thermostat)
static size_t tagged_words_allocated() { return (size_t)2 * GRID_CAP * CHAIN_INLINE_SUM_NT; }
static size_t tagged_words_touched(int grid, int NT) {
    if (grid < 1) return 0;
    const int r = grid - 1, j = 2 * NT - 1;
    return ((size_t)(r >> 6) * (2 * CHAIN_INLINE_SUM_NT) + j) * 64 + (r & 63) + 1;
}

// The sizes a streaming launch is bound by, checked on the host before it goes out: one row of partial sums per work-group
// in a table of GRID_CAP rows; tagged rows only with G <= 8; a wave-tile table of num_wtiles + 1 entries in which every tile
// holds <= 64 slots (tgnh_create built them so: this is the launch-side half of that contract).
static tgnh_status check_launch(tgnh_handle h, const TileArgs& a, int grid, int block, bool wave, bool tagged) {
    if (grid < 1 || grid > GRID_CAP || grid > h->cfg.grid) return fail(TGNH_ERR_STATE, "internal: grid exceeds the partial-row table");
    if (wave) {
        if (!a.wave_tile || (int)h->topo.wave_tile.size() != a.num_wtiles + 1 || a.num_wtiles < 1)
            return fail(TGNH_ERR_STATE, "internal: wave-tile table does not match the launch");
        if ((long long)grid * (block / 64) > (long long)a.num_wtiles + (block / 64) - 1)
            return fail(TGNH_ERR_STATE, "internal: more work-groups than wave tiles");
    } else if (grid > h->topo.num_tiles) return fail(TGNH_ERR_STATE, "internal: more work-groups than tiles");
    if (tagged) {
        if (!a.rows || !a.sync || h->thermo.L.NT > CHAIN_INLINE_SUM_NT || tagged_words_touched(grid, h->thermo.L.NT) > tagged_words_allocated())
            return fail(TGNH_ERR_STATE, "internal: tagged rows do not fit their area");
    }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_launch_bounds(tgnh_handle h, int32_t out[8]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    const int nw = h->topo.num_wtiles;
    int g = h->topo.num_tiles;                                                    // tile_kernel / step_kernel: at most one work-group per tile
    if (nw > 0) g = std::max(g, (nw + TBLOCK / 64 - 1) / (TBLOCK / 64));     // wke_kernel: per four wave tiles (wstep_kernel: per eight)
    g = std::max(1, std::min(g, GRID_CAP));
    const bool tagged = h->thermo.L.NT <= CHAIN_INLINE_SUM_NT && (h->meet.d_rows != nullptr || h->host_only);
    out[0] = h->topo.num_tiles; out[1] = nw; out[2] = (int)h->topo.wave_tile.size(); out[3] = g;
    out[4] = h->cfg.grid; out[5] = tagged ? (int)tagged_words_allocated() : 0;
    out[6] = tagged ? (int)tagged_words_touched(g, h->thermo.L.NT) : 0; out[7] = h->thermo.L.NT;
    return TGNH_OK;
}

tgnh_status run_big_com(tgnh_handle h, bool kick, hipStream_t s) {
    BigComArgs b{};
    b.table = h->topo.d_big_table; b.n = h->topo.num_big; b.velm = h->bound.velm;
    b.force = reinterpret_cast<const long long*>(h->bound.force); b.padded = h->d.padded_num_particles;
    b.kick = kick ? 1 : 0; b.dt = h->d.step_size;
    b.big_com = h->topo.d_big_com;
    b.partials = h->thermo.d_partials + (size_t)GRID_CAP * h->thermo.L.NT; b.NT = h->thermo.L.NT; b.G = h->thermo.L.G;
    Timed t(h, s, KID_OTHER);
    HIP_OK(launch_big_com(h->d.precision, b, s));
    return TGNH_OK;
}

// ---- the gather path (tgnh_gather.hip): the same operation masks, by global index ----
GatherArgs gather_args(tgnh_handle h, const double* scale) {
    GatherArgs a = common_args<GatherArgs>(h, scale);
    a.group = h->gather.d_group; a.resid = h->gather.d_resid;
    a.res_table = h->gather.d_res_table; a.partner = h->gather.d_partner; a.com = h->gather.d_com;
    a.n = h->d.num_particles;
    a.com_lanes = h->gather.com_lanes;
    a.n_res = a.use_com ? (int)h->gather.res_table.size() : 0;
    a.G = h->thermo.L.G; a.NT = h->thermo.L.NT;
    return a;
}

// One operation mask of run_tile as launches of the gather kernels: the velocity / position part (rescale, kick, drift,
// posDelta, move, hard wall) first, the kinetic energies of what it stored after it (K's order: Cu :384-388 then :474-488).
static tgnh_status run_gather(tgnh_handle h, int ops, int kid, hipStream_t s, const double* scale) {
    GatherArgs a = gather_args(h, scale);
    if ((ops & (OP_POSDELTA | OP_MOVE)) && !h->bound.pos_delta) return fail(TGNH_ERR_STATE, "posDelta buffer not bound");
    const int upd = ops & (OP_SCALE | OP_KICK | OP_DRIFT | OP_POSDELTA | OP_MOVE | OP_PREKICK);
    if (ops & OP_NOSTORE) return fail(TGNH_ERR_STATE, "internal: the gather path stores every kick");
    Timed t(h, s, kid);
    if (upd) {
        // K :474-479 before :351-353: v - v_com of the velocities about to be rescaled.  On this path every rescale follows a
        // kinetic-energy pass and its chain inside one entry point (the flags that would part them are ignored), so the table
        // that pass left is of these very velocities: not computed again
        if ((upd & OP_SCALE) && a.use_com && !(h->owed.g_com_fresh && !(upd & OP_PREKICK))) {
            a.kick_com = (upd & OP_PREKICK) ? 1 : 0;
            HIP_OK(launch_gather_com(h->d.precision, a, s));
        }
        h->owed.g_com_fresh = false;
        a.ops = upd;
        HIP_OK(launch_gather_update(h->d.precision, a, s));
    }
    if (ops & OP_KE) {
        a.kick_com = 0;
        if (a.use_com) HIP_OK(launch_gather_com(h->d.precision, a, s));
        const int grid = gather_ke_grid(a);
        HIP_OK(launch_gather_ke(h->d.precision, a, grid, s));
        h->run.ke_parts = grid;
        h->owed.tail_summed = false;
        h->owed.g_com_fresh = a.use_com != 0;
    }
    return TGNH_OK;
}

// sum the rows of the gather path's kinetic-energy kernel [+ all-reduce], run the chain: more than 34 thermostats / long links
tgnh_status run_chain_gather(tgnh_handle h, hipStream_t s, bool sum_only) {
    ChainArgs a = chain_args(h);
    Timed t(h, s, KID_CHAIN);
    HIP_OK(launch_gather_rowsum(h->thermo.d_partials, h->run.ke_parts, h->thermo.L.NT, h->thermo.d_state + h->thermo.L.off_ke_red, s));
    { tgnh_status rc = allreduce_hook(h, s); if (rc) return rc; }
    if (!sum_only) HIP_OK(launch_gather_chain(a, h->gather.d_scratch, s));
    return TGNH_OK;
}

// run_tile, part 1.  A rescale launch that finds a chain waiting runs it itself: its chain wavefronts read the thermostat block
// st_in, work-group 0 leaves the advanced one in st_out: d_state -> d_stage, for whoever comes next to commit.  A carried chain
// (no KE pass before it: nothing has committed the staged block on the way) reads the thermostat where the last in-kernel chain
// left it and writes the other copy: the two blocks differ only in what a chain writes, and a chain writes all of that every time
// (eta, etaDot, etaDotDot, KE before / after, the scale factors, KESum)
static tgnh_status adopt_chain(tgnh_handle h, TileArgs& a, hipStream_t s) {
    const bool pingpong = h->owed.carry_pending && h->owed.stage_pending;
    if (h->owed.stage_pending && !pingpong) { tgnh_status rc = commit_stage(h, s); if (rc) return rc; }
    a.chain_on = 1;
    a.chain = chain_args(h);                                    // (takes note of the staged block: cleared there)
    a.chain.chain_twice = h->owed.chain_pending_twice ? 1 : 0;
    a.chain.ke_carry = h->owed.carry_pending ? 1 : 0;
    a.sum_rows = h->owed.sum_pending ? (h->run.ke_parts + h->topo.num_big <= h->cfg.inline_sum_rows ? 1 : 2) : 0;
    a.x_wait = h->owed.xwait_pending ? 1 : 0;
    a.st_in = pingpong ? h->thermo.d_stage : h->thermo.d_state;
    a.st_out = pingpong ? h->thermo.d_state : h->thermo.d_stage;
    return TGNH_OK;
}

// run_tile, part 2.  What a KE pass of `grid` work-groups does besides reducing: it commits a staged thermostat block on the
// way; on wave tiles its work-group 0 sums the rows where a launch that only did that would follow (an all-reduce waits for the
// sums, or the next rescale launch does not sum them); the COM velocities of the big molecules are tabulated first, for the
// velocities this launch reduces: the current ones, or the kicked ones (the kick is linear, so sum m v' = sum (m v + dt/2 F)
// needs no second pass).  The rescale launches that follow reuse the table: velocities do not change between a KE pass and its rescale.
static tgnh_status ke_pass_prologue(tgnh_handle h, TileArgs& a, int ops, bool wave, int grid, hipStream_t s) {
    if (h->owed.stage_pending && !a.chain_on) {
        a.commit_len = h->thermo.L.total; a.commit_src = h->thermo.d_stage; a.commit_dst = h->thermo.d_state;
        a.commit_skip = h->thermo.L.off_ke_red; a.commit_skip_n = h->thermo.L.NT;
        h->owed.stage_pending = false;
    }
    h->owed.tail_summed = wave && h->meet.d_rows && !h->xchg.on && h->thermo.L.NT <= CHAIN_INLINE_SUM_NT && !rescale_sums_rows(h, grid);
    if (h->owed.tail_summed) { a.tail_sum = 1; a.rows = h->meet.d_rows; a.sync = h->meet.d_sync; a.ke_red = h->thermo.d_state + h->thermo.L.off_ke_red; }
    h->run.ke_parts = grid;
    return big_com_on(h) ? run_big_com(h, (ops & OP_KICK) != 0, s) : TGNH_OK;
}

// run_tile, part 3: the launch, its sizes checked first
static tgnh_status launch_pass(tgnh_handle h, int ops, int kid, const TileArgs& a, bool wave, int grid, size_t lds, hipStream_t s) {
    tgnh_status rc = check_launch(h, a, grid, TBLOCK, wave, a.tail_sum != 0); if (rc) return rc;
    Timed t(h, s, kid);
    if (wave) HIP_OK(launch_wke(h->d.precision, ops, h->cfg.gb, a, grid, s));
    else HIP_OK(launch_tile(h->d.precision, ops, h->cfg.gb, a, grid, lds, s));
    return TGNH_OK;
}

// One streaming launch with the operation mask `ops` (scale != nullptr: these factors, and no chain is adopted)
tgnh_status run_tile(tgnh_handle h, int ops, int kid, hipStream_t s, const double* scale) {
    if (h->gather.generic) return run_gather(h, ops, kid, s, scale);
    tgnh_status rc;
    TileArgs a = tile_args(h, scale);
    if ((ops & OP_SCALE) && h->owed.chain_pending && !scale) { rc = adopt_chain(h, a, s); if (rc) return rc; }
    if ((ops & (OP_POSDELTA | OP_MOVE)) && !h->bound.pos_delta) return fail(TGNH_ERR_STATE, "posDelta buffer not bound");
    size_t lds = tile_lds_bytes(h->d.precision, ops, a.hardwall != 0, a.use_com != 0);
    if ((ops & OP_KE) && h->cfg.gb == 0) lds += sizeof(double) * (TBLOCK / 64) * h->thermo.L.G;   // per-wave group bins
    // the pure KE passes (KE, kick+KE, kick+KE unstored) run over the wave tiles when the topology has them
    const bool wave = h->cfg.wave_ke && (ops & OP_KE) && !(ops & ~(OP_KE | OP_KICK | OP_NOSTORE));
    const int grid = wave ? wave_grid_for(h, ops) : grid_for(h, ops, a.hardwall != 0, lds);
    if (ops & OP_KE) { rc = ke_pass_prologue(h, a, ops, wave, grid, s); if (rc) return rc; }
    rc = launch_pass(h, ops, kid, a, wave, grid, lds, s); if (rc) return rc;
    if (a.chain_on) { h->owed.chain_ran(); h->owed.stage_pending = a.st_out == h->thermo.d_stage; }    // the advanced thermostat lies where the launch wrote it
    if (h->cfg.alternate_sweeps) h->run.sweep_reverse ^= 1;      // the next streaming launch starts where this one ends
    return TGNH_OK;
}

ChainArgs chain_args(tgnh_handle h) {
    ChainArgs a{};
    a.L = h->thermo.L; a.st = h->thermo.d_state; a.partials = h->thermo.d_partials; a.nparts = h->run.ke_parts;
    a.nbig = h->topo.num_big;
    a.dt = h->d.step_size; a.S = h->d.drude_steps_per_real_step;
    a.dtc = a.dt / a.S; a.inv_dtc = 1.0 / a.dtc;                               // Cu :440-443
    a.realkbT = h->thermo.realkbT; a.drudekbT = h->thermo.drudekbT;
    a.stage = h->thermo.d_stage;
    a.status = h->status.d_word;
    if (h->xchg.on) a.x = h->xchg.args;
    a.commit = h->owed.stage_pending ? 1 : 0;     // every chain_kernel launch takes over a staged block first
    h->owed.stage_pending = false;
    return a;
}

// a staged block with no chain_kernel launch coming up: commit it by a launch that does nothing else
static tgnh_status commit_stage(tgnh_handle h, hipStream_t s) {
    if (!h->owed.stage_pending) return TGNH_OK;
    ChainArgs a = chain_args(h);
    a.do_sum = 0; a.do_chain = 0;
    HIP_OK(launch_chain(a, s));
    return TGNH_OK;
}

// Between a KE pass and the rescale that uses its factors: sum the work-group partials, exchange the sums across ranks when
// sharded, run the chain.  Three answers, settled first, say what of that is launched here:
//   who sums the rows     the KE launch's tail sum did (ke_pass_prologue) | a launch now | the next rescale launch (rescale_sums_rows)
//   which exchange        none | the hook, after the sums | the mailboxes: the row-sum launch sends, whoever runs the chain waits
//   where the chain runs  in a launch now | inside the next rescale launch (cfg.inline_chain: 1-4 links)
//   handle                                rows              exchange    chain
//   1-4 links, unsharded, <= 8 groups     next rescale      none        next rescale      (nothing launched: 3 launches per step)
//   1-4 links, unsharded, more groups     tail sum | now    none        next rescale
//   1-4 links, hook                       tail sum | now    hook        next rescale
//   1-4 links, mailboxes                  now               mailboxes   next rescale
//   5+ links, unsharded                   tail sum | now    none        now, in the row-sum launch (one launch also after a tail sum)
//   5+ links, hook                        tail sum | now    hook        now, in a launch of its own behind the hook
//   5+ links, mailboxes                   now               mailboxes   now, in the row-sum launch
// (After a tail sum ke_red is complete, and nothing is staged: a KE launch commits.  The gather path's own chain: run_chain_gather.)
// Where the rescale launch sums: up to 256 rows its chain wavefront reads them alone (one batch of loads); more rows are read by
// all four wavefronts, a quarter each, ahead of their tile loads (read by one wavefront they were a chain of L2 misses on the
// critical path, +7-9 us) -- that up to 2 M slots (inline_sum_all).  +4 % steps/s at 625 k slots, +7-17 % for small systems
// (profiles/r01_tuning_sweep.log).
static tgnh_status run_chain(tgnh_handle h, hipStream_t s, bool twice) {
    if (h->gather.chain) return run_chain_gather(h, s, false);
    const bool sum_next = rescale_sums_rows(h, h->run.ke_parts), sum_now = !sum_next && !h->owed.tail_summed;
    const bool mailbox = h->xchg.on, hook = !mailbox && h->xchg.allreduce;
    const bool chain_next = h->cfg.inline_chain;                                  // (sum_next implies it)
    const bool chain_with_sum = !chain_next && !hook, chain_alone = !chain_next && hook;
    h->owed.tail_summed = false;
    tgnh_status rc;
    ChainArgs a = chain_args(h);
    a.chain_twice = twice ? 1 : 0;
    if (sum_now || chain_with_sum) {
        a.do_sum = sum_now ? 1 : 0; a.x_send = mailbox ? 1 : 0;
        a.do_chain = chain_with_sum ? 1 : 0; a.x_wait = mailbox && chain_with_sum ? 1 : 0;
        rc = timed_chain(h, a, s); if (rc) return rc;
    }
    if (hook) { rc = allreduce_hook(h, s); if (rc) return rc; }
    if (chain_alone) {
        a.do_sum = 0; a.do_chain = 1; a.commit = 0;
        rc = timed_chain(h, a, s); if (rc) return rc;
    }
    if (chain_next) { h->owed.chain_owed(twice); h->owed.sum_pending |= sum_next; h->owed.xwait_pending |= mailbox; }
    return TGNH_OK;
}

// a chain that is still waiting for its rescale launch is run now, in place, by the standalone kernel
tgnh_status materialize_chain(tgnh_handle h, hipStream_t s) {
    { tgnh_status rc = settle_end(h, s); if (rc) return rc; }
    if (!h->owed.chain_pending) return commit_stage(h, s);
    ChainArgs a = chain_args(h);
    a.do_sum = h->owed.sum_pending ? 1 : 0; a.do_chain = 1; a.chain_twice = h->owed.chain_pending_twice ? 1 : 0;
    a.x_wait = h->owed.xwait_pending ? 1 : 0;
    a.ke_carry = h->owed.carry_pending ? 1 : 0;
    { tgnh_status rc = timed_chain(h, a, s); if (rc) return rc; }
    h->owed.chain_ran();
    return TGNH_OK;
}

// ---- TGNH_FLAG_RESIDENT_STEP: one launch per time step (step_kernel) ----
// Eligible: deferred pass structure, one-link chains (the chain runs inside the launch), at most 8 temperature groups,
// and an exchange the kernel can do itself (none, or the mailboxes -- a collective hook is a launch of its own).
// -> 0: none (the launches), 1: step_kernel, 2: wstep_kernel
static int resident_kernel(tgnh_handle h, int kind) {
    if (!((h->d.flags & TGNH_FLAG_RESIDENT_STEP) && h->cfg.inline_chain && h->cfg.gb != 0 && h->thermo.L.NT <= CHAIN_INLINE_SUM_NT &&
          (h->xchg.on || !h->xchg.allreduce))) return 0;
    if (kind == 0 && h->cfg.wresident_per_cu > 0) return 2;              // wstep_kernel: a whole deferred step over wave tiles, chains of 1-4 links
    return h->cfg.resident_per_cu > 0 && h->thermo.L.C == 1 ? 1 : 0;           // step_kernel: every kind, one-link chains
}
bool resident_now(tgnh_handle h) { return resident_kernel(h, pass_kind(h->d)) != 0; }

extern "C" tgnh_status tgnh_get_step_path(tgnh_handle h, int* gather, const char** reason) {
    CHECK_H(h);
    if (gather) *gather = h->gather.generic ? (h->gather.chain ? 2 : 1) : 0;
    if (reason) *reason = h->gather.reason.c_str();
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_resident_kernel(tgnh_handle h, int* which) {
    CHECK_H(h);
    if (!which) return fail(TGNH_ERR_ARG, "null out");
    *which = resident_kernel(h, pass_kind(h->d));
    return TGNH_OK;
}

// ---- wstep_kernel's velocities as three planes (tgnh_vplanes.hip) ----
// Between the steps of a DEFER_SCALE | RESIDENT_STEP sequence velm is stale by contract (owed.end_pending), and everybody who
// needs real velocities comes through settle_end.  So between two settles the library may keep the velocities where the kernel
// moves fewest bytes: x | y | z planes of its own, without the 1/m word and without the massless slots (owed.planes_live;
// VelPlanes in tgnh_context.h).  Both layouts give the same bits: where the velocities live changes no result, only the bytes a
// step moves.
//
// Entered by the one-launch step after PLANES_AFTER_STEPS such steps in a row since the last settle.  By the bytes (arithmetic, not
// a measurement; mixed precision, f = the box's share of massive slots, 4/5 for SWM4 water): the two conversions of one stay move
// (32 + 24 f) + (24 f + 64 f) B per slot -- 121.6 for water, 144 where every slot has mass -- and a step there saves 96 - 72 f
// of velm's 96 B of V -- 38.4 for water, 24 where every slot has mass --, so a stay pays from its fourth step (water) to its seventh.
// A caller that settles every step never reaches the threshold and never converts; one that settles every 100 steps or more -- a
// reporter -- loses the gain of 8 steps in 100; the worst case, a settle every 10 steps, converts for one step on the planes and is
// 4 % of its ten steps' bytes slower.  The threshold stays where the full planes put it (tests read it).
constexpr int PLANES_AFTER_STEPS = 8;

// planes -> velm (no Timed scope: tests/test_launch_structure_gpu.py counts the scopes of a settle)
static tgnh_status leave_planes(tgnh_handle h, hipStream_t s) {
    if (!h->owed.planes_live) return TGNH_OK;
    HIP_OK(launch_planes_to_velm(h->d.precision, h->vp.d_planes, h->bound.velm, h->topo.d_wave_tile, h->topo.num_wtiles, h->vp.d_invm,
                                 h->vp.d_base, h->vp.d_off, h->vp.stride, s));
    h->owed.planes_live = false;
    return TGNH_OK;
}

// velm -> planes, when the one-launch step about to go out is due to run on them.  Never inside a stream capture: a conversion
// baked into a graph would be replayed from stale data, and the first conversion of a bind waits for the device (it checks that
// the inverse masses the kernel will take from its pattern table are velm's w, bit for bit; the verdict is kept).  Steps
// recorded while velm holds the velocities pin the handle there: their graph may be replayed between eager steps for good.
static tgnh_status enter_planes(tgnh_handle h, hipStream_t s) {
    tgnh_context::VelPlanes& vp = h->vp;
    if (h->owed.planes_live || !vp.usable()) return TGNH_OK;
    if (stream_capturing(s)) { vp.pinned = true; return TGNH_OK; }
    if (vp.streak < PLANES_AFTER_STEPS) return TGNH_OK;
    const bool check = vp.verdict == 0;
    if (check) HIP_OK(hipMemsetAsync(vp.d_mismatch, 0, sizeof(uint32_t), s));
    HIP_OK(launch_velm_to_planes(h->d.precision, h->bound.velm, vp.d_planes, h->topo.d_wave_tile, h->topo.num_wtiles, vp.d_invm,
                                 vp.d_base, vp.d_off, vp.stride, check ? vp.d_mismatch.get() : nullptr, s));
    if (check) {
        uint32_t differs = 1;
        HIP_OK(hipMemcpyAsync(&differs, vp.d_mismatch, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        vp.verdict = differs ? -1 : 1;
        if (differs) return TGNH_OK;                        // some w is not 1 / (descriptor mass) as the table has it: velm it stays, same results
    }
    h->owed.planes_live = true;
    return TGNH_OK;
}

// velm holds what the handle's other flags say it holds: planes that a one-launch step left live with nothing else pending
// (between tgnh_step_begin and tgnh_step_end) are written back.  For the entry points that touch velm without settling anything.
tgnh_status velm_current(tgnh_handle h, hipStream_t s) {
    return h->owed.planes_live && !h->owed.end_pending ? settle_end(h, s) : TGNH_OK;
}

extern "C" tgnh_status tgnh_get_velocity_planes(tgnh_handle h, int32_t out[4]) {
    CHECK_H(h);
    if (!out) return fail(TGNH_ERR_ARG, "null out");
    out[0] = h->owed.planes_live ? 1 : 0; out[1] = h->vp.usable() ? 1 : 0; out[2] = h->vp.streak; out[3] = PLANES_AFTER_STEPS;
    return TGNH_OK;
}

// One launch of step_kernel.  kind 0: a whole deferred step (the last step's end half + this step's begin half, both chain
// halves); 1 / 2: the begin / end half of the reference's pass structure; 3 / 4: the same around the constraint call-outs.
static tgnh_status run_resident(tgnh_handle h, hipStream_t s, int kind) {
    if (h->owed.stage_pending) { tgnh_status rc = commit_stage(h, s); if (rc) return rc; }
    const bool wstep = resident_kernel(h, kind) == 2;
    // where this launch finds the velocities (only the one-launch step ever leaves them in the planes, and every other way to a
    // launch goes through settle_end first: tgnh_step_begin, second_half, split_entry)
    if (wstep && kind == 0) { tgnh_status rc = enter_planes(h, s); if (rc) return rc; }
    else if (h->owed.planes_live) return fail(TGNH_ERR_STATE, "internal: a launch that reads velm while the velocities live in the planes");
    TileArgs a = tile_args(h, nullptr);
    if (h->owed.planes_live) {
        a.vplanes = h->vp.d_planes; a.wpat_invm = h->vp.d_invm; a.wtile_base = h->vp.d_base; a.wpat_off = h->vp.d_off; a.vstride = h->vp.stride;
        h->vp.stream = s;
    }
    const int ops2 = step_kind_ops2(kind);
    if ((ops2 & OP_POSDELTA) && !h->bound.pos_delta) return fail(TGNH_ERR_STATE, "posDelta buffer not bound");
    const bool hw = a.hardwall != 0 && (ops2 & (OP_DRIFT | OP_MOVE));
    const size_t lds = tile_lds_bytes(h->d.precision, ops2, hw, a.use_com != 0);
    int& grid = h->cfg.resident_grid[kind][hw ? 1 : 0];
    if (grid == 0 && !wstep) {       // the work-groups that are resident at once (counted at create; never more than this kind's own occupancy)
        int per_cu = std::min(h->cfg.resident_per_cu, step_blocks_per_cu(h->d.precision, h->cfg.gb, kind, lds));
        if (per_cu < 1) return fail(TGNH_ERR_HIP, "step_kernel: occupancy query failed");
        grid = std::max(1, std::min(std::min(h->topo.num_tiles, per_cu * h->cfg.num_cus / h->cfg.resident_share), GRID_CAP));
    }
    a.chain_on = 1;
    a.chain = chain_args(h);
    a.chain.chain_twice = kind == 0 ? 1 : 0;
    a.x_wait = 1;
    if (!h->xchg.on) a.chain.x = h->meet.self_x;            // unsharded: the private one-rank mailbox
    a.st_in = h->thermo.d_state; a.st_out = h->thermo.d_state;       // advanced in place by work-group 0 after everybody has read it
    a.sync = h->meet.d_sync; a.rows = h->meet.d_rows;
    if (big_com_on(h)) { tgnh_status rc = run_big_com(h, kind == 0 || kind == 2, s); if (rc) return rc; }
    if (wstep && h->cfg.wresident_grid == 0) {                 // a whole deferred step over wave tiles (wstep_kernel)
        const int need = (h->topo.num_wtiles + WBLOCK / 64 - 1) / (WBLOCK / 64);
        h->cfg.wresident_grid = std::max(1, std::min(std::min(need, h->cfg.wresident_per_cu * h->cfg.num_cus / h->cfg.resident_share), GRID_CAP));
    }
    const int g = wstep ? h->cfg.wresident_grid : grid;
    a.chain.nparts = g;
    h->run.ke_parts = g;
    { tgnh_status rc = check_launch(h, a, g, wstep ? WBLOCK : TBLOCK, wstep, true); if (rc) return rc; }
    {
        Timed t(h, s, KID_STEP);
        if (wstep) HIP_OK(launch_wstep(h->d.precision, h->cfg.gb, h->thermo.L.C > 1, a, g, s));
        else HIP_OK(launch_step(h->d.precision, h->cfg.gb, kind, a, g, lds, s));
    }
    // the first pass walked the tiles in direction sweep_reverse, the second one back: the next launch starts here
    h->owed.resident_settled();
    if (wstep && kind == 0 && h->vp.usable()) h->vp.streak = std::min(h->vp.streak + 1, 1 << 30);         // (enter_planes' count; a recording on velm has pinned the handle and counts nothing)
    return TGNH_OK;
}

// make scale[] hold the first thermostat half step for the current velocities (Ref :231, Cu :336)
static tgnh_status first_half(tgnh_handle h, hipStream_t s) {
    if (h->owed.first_half_done) return TGNH_OK;               // DEFER_SCALE: already folded into scale[]
    if (h->owed.ke_carry) {
        // TRUST_STATE_CHANGED, and nothing has written velocities since the last end half's rescale: every kinetic-energy bin
        // of the stored velocities is s^2 times the bin that chain started from -- the ke_post it left (Cu :574 tracks exactly
        // that product) -- so this half's KE pass (Cu :474-488) and its row sum are not run: the chain starts from ke_post
        h->owed.ke_carry = false;
        // (molecules longer than a tile: the KE pass that is not run would have left their centre-of-mass velocities in
        // the table the rescale launch reads -- the end half's rescale has changed them since)
        if (big_com_on(h)) { tgnh_status rc = run_big_com(h, false, s); if (rc) return rc; }
        if (h->cfg.inline_chain) {                            // ... inside the rescale launch that follows: this half step is ONE launch
            h->owed.chain_owed(false); h->owed.sum_pending = false; h->owed.carry_pending = true;
            return TGNH_OK;
        }
        ChainArgs a = chain_args(h);
        a.do_sum = 0; a.do_chain = 1; a.ke_carry = 1;
        return timed_chain(h, a, s);
    }
    tgnh_status rc = run_tile(h, OP_KE, KID_KE, s); if (rc) return rc;
    return run_chain(h, s, false);
}

// Every entry point that launches work or hands results back starts here: a failure the device reported earlier
// (a mailbox exchange that timed out; in dualNH mode a Drude beyond twice the hard wall, Ref :311-312) is sticky --
// the trajectory is no longer the integrator's, so nothing more is computed on it.
tgnh_status entry(tgnh_handle h, bool need_bufs) {
    if (!h) return fail(TGNH_ERR_ARG, "null handle");
    h->owed.g_com_fresh = false;                                           // (the caller may have written velocities since the last entry point)
    if (need_bufs) { tgnh_status rc = need_buffers(h); if (rc) return rc; }
    if (!h->host_only) {
        HIP_OK(hipSetDevice(h->device));
        if (h->status.h_seen) note_status(h, *h->status.h_seen);     // the last periodic read-back, if it has landed
    }
    if (h->status.failed_code) return fail(h->status.failed_code, h->status.failed);
    return TGNH_OK;
}

// Every STATUS_POLL_EVERY steps the status word is copied to pinned host memory behind the step (no synchronisation;
// looked at on a later entry): a caller that never asks for anything still learns of a failure within that many steps.
static tgnh_status poll_status_async(tgnh_handle h, hipStream_t s) {
    if (!h->status.h_seen || h->run.step_count % STATUS_POLL_EVERY != 0) return TGNH_OK;
    if (stream_capturing(s)) return TGNH_OK;
    HIP_OK(hipMemcpyAsync(h->status.h_seen, h->status.d_word, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return TGNH_OK;
}

// Consecutive streaming launches sweep the slots in alternating directions (a launch starts where the last one ended), and
// the direction decides the order in which a wavefront adds its tiles' kinetic energies, i.e. the last bits of the sums.  A
// time step holds an odd number of sweeps in every pass structure, so in an undisturbed run step k starts in direction k & 1;
// that is made the rule: whatever was launched between two steps (queries, a flush), a step starts in the direction of
// its number.  The trajectory's bits are then a function of the state and the step counter alone -- a handle restored from a
// checkpoint (tgnh_set_time carries the counter) continues bit for bit, ranks of a sharded run sweep alike.
static void start_of_step(tgnh_handle h) {
    if (h->cfg.alternate_sweeps) h->run.sweep_reverse = (int)(h->run.step_count & 1);
}
// ... and the end of one                                                          Cu :405-406 ; Ref :413-414
static tgnh_status advance_clock(tgnh_handle h, hipStream_t s) {
    h->run.time += h->d.step_size; h->run.step_count += 1;
    return poll_status_async(h, s);
}

extern "C" tgnh_status tgnh_step_begin(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = cm_removal_due(h, s); if (rc) return rc;
    rc = rescale_due(h, s); if (rc) return rc;
    start_of_step(h);
    if (h->owed.end_pending && resident_now(h)) return run_resident(h, s, 0);      // the last step's end half and this begin half: one launch
    rc = settle_end(h, s); if (rc) return rc;                        // (an end half that waits; velocity planes a step without an end half left live)
    if (!(h->d.flags & TGNH_FLAG_DEFER_SCALE) && resident_now(h) && !h->owed.ke_carry)
        return run_resident(h, s, 1);                                // reference pass structure: KE, chain, rescale+kick+drift in one launch
    rc = first_half(h, s); if (rc) return rc;                       // (kinetic energies carried over: no first pass, no meeting -- the tile launch with its in-kernel chain)
    // Cu :351-376 fused; with a half kick still pending from the last step_end (DEFER_SCALE) that kick comes first
    rc = run_tile(h, (h->owed.kick_pending ? OP_PREKICK : 0) | OP_SCALE | OP_KICK | OP_DRIFT, KID_SKD, s); if (rc) return rc;
    h->owed.velocities_current(); h->owed.first_half_done = false;
    return TGNH_OK;
}

static tgnh_status second_half(tgnh_handle h, hipStream_t s, int kick_ops) {
    tgnh_status rc;
    const bool defer = (h->d.flags & TGNH_FLAG_DEFER_SCALE) != 0;
    h->owed.ke_carry = false;                                   // (an end half without a begin half before it: its own KE pass runs in any case)
    if (h->owed.scale_pending || h->owed.kick_pending || h->owed.end_pending) { rc = flush_impl(h, s); if (rc) return rc; }   // two end halves in a row
    if (!(defer && kick_ops && resident_now(h))) { rc = velm_current(h, s); if (rc) return rc; }     // (every branch but the one that launches nothing reads velm)
    if (!defer && resident_now(h)) {
        // reference pass structure: kick, KE, chain, rescale (Cu :384-402) in one launch; velocities are final when it ends
        rc = run_resident(h, s, kick_ops ? 2 : 4); if (rc) return rc;
        h->owed.ke_carry = ke_carries(h);
    } else if (kick_ops && resident_now(h)) {
        // TGNH_FLAG_RESIDENT_STEP: nothing is launched here -- the next tgnh_step_begin runs this end half and its own
        // begin half in one launch (step_kernel); anything that needs the state earlier settles it the classic way
        h->owed.end_pending = true;
    } else {
        // DEFER_SCALE, fused path: the kicked velocities only feed the sums (Cu :384-388 + :474-488); the next step's first
        // launch -- or tgnh_flush -- forms them again from the same force buffer and goes on from there.
        // The reference's own structure, fused path (round 4): the same unstored kick+KE pass, and the rescale launch of THIS call forms
        // the kicked velocities again before it rescales them (OP_PREKICK: the same expression on the same force buffer, the same
        // bits) -- V r, F r | V r/w, F r = 144 B per slot where kick+KE with a store and a plain rescale move 152, and the read-only
        // pass runs at 62 us where the storing one takes 87-92 (5 M slots).  velm holds the reference's end-of-step velocities when
        // tgnh_step_end returns, as before.  (The split path's halves work on stored velocities around the constraint call-outs.)
        const bool fold = !defer && kick_ops != 0 && !h->gather.generic;           // (the gather path stores its kick: K's own structure)
        const int nostore = kick_ops && !h->gather.generic ? OP_NOSTORE : 0;
        h->owed.end_folded = fold;
        rc = run_tile(h, kick_ops | OP_KE | nostore, kick_ops ? KID_KICK_KE : KID_KE, s); if (rc) return rc;
        rc = run_chain(h, s, defer); if (rc) return rc;                                // Cu :394-395
        if (defer) h->owed.end_half_deferred(nostore != 0);
        else {
            rc = run_tile(h, (fold ? OP_PREKICK : 0) | OP_SCALE, KID_SCALE, s); if (rc) return rc;   // Cu :402 (and :384-388 again, see above)
            h->owed.ke_carry = ke_carries(h);
        }
    }
    return advance_clock(h, s);
}

extern "C" tgnh_status tgnh_step_end(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    return second_half(h, (hipStream_t)stream, OP_KICK);
}

// The split entry points work on stored velocities: a deferred half kick is materialised first.
tgnh_status settle_kick(tgnh_handle h, hipStream_t s) {
    return (h->owed.kick_pending || h->owed.end_pending || h->owed.planes_live) ? flush_impl(h, s) : TGNH_OK;
}

// TGNH_FLAG_RESIDENT_STEP left the end half of the last step to the next tgnh_step_begin; somebody needs it now:
// the classic launches (kick+KE without a velocity store, row sum [+ exchange], both chain halves pending)
// Velocities that live in the library's planes go back to velm first -- here and nowhere else -- and the count towards the next
// stay on them starts again.
tgnh_status settle_end(tgnh_handle h, hipStream_t s) {
    if (h->owed.planes_live || h->owed.end_pending) h->vp.streak = 0;
    tgnh_status rc = leave_planes(h, s); if (rc) return rc;
    if (!h->owed.end_pending) return TGNH_OK;
    h->owed.end_pending = false;
    rc = run_tile(h, OP_KICK | OP_KE | OP_NOSTORE, KID_KICK_KE, s); if (rc) return rc;
    rc = run_chain(h, s, true); if (rc) return rc;
    h->owed.end_half_deferred(true);
    return TGNH_OK;
}

// ... so every one of them begins like this.  fresh_ke: what it is about to do writes velocities or positions behind the
// carried kinetic energies' back
static tgnh_status split_entry(tgnh_handle h, hipStream_t s, bool fresh_ke) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    if (fresh_ke) h->owed.ke_carry = false;
    return settle_kick(h, s);
}

extern "C" tgnh_status tgnh_step_begin_kick(tgnh_handle h, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    tgnh_status rc = split_entry(h, s, false); if (rc) return rc;
    rc = cm_removal_due(h, s); if (rc) return rc;
    rc = rescale_due(h, s); if (rc) return rc;
    start_of_step(h);
    if (!(h->d.flags & TGNH_FLAG_DEFER_SCALE) && resident_now(h) && !h->owed.ke_carry) return run_resident(h, s, 3);
    rc = first_half(h, s); if (rc) return rc;
    rc = run_tile(h, OP_SCALE | OP_KICK | OP_POSDELTA, KID_OTHER, s); if (rc) return rc;   // Cu :351-360
    h->owed.scale_pending = false; h->owed.first_half_done = false;
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_step_begin_move(tgnh_handle h, void* stream) {
    tgnh_status rc = split_entry(h, (hipStream_t)stream, true); if (rc) return rc;
    return run_tile(h, OP_MOVE, KID_OTHER, (hipStream_t)stream);                   // Cu :366-376
}
extern "C" tgnh_status tgnh_step_end_kick(tgnh_handle h, void* stream) {
    tgnh_status rc = split_entry(h, (hipStream_t)stream, true); if (rc) return rc;
    return run_tile(h, OP_KICK, KID_OTHER, (hipStream_t)stream);                   // Cu :384-388
}
extern "C" tgnh_status tgnh_step_end_thermo(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    return second_half(h, (hipStream_t)stream, 0);                                 // Cu :394-406
}
extern "C" tgnh_status tgnh_half_kick(tgnh_handle h, void* stream) { return tgnh_step_end_kick(h, stream); }

// velm <- the reference's end-of-step velocities: the pending half kick (same force buffer), then the end-of-step
// factors; scale[] keeps only the pre-run first half of the coming step
tgnh_status flush_impl(tgnh_handle h, hipStream_t s) {
    tgnh_status rc = settle_end(h, s); if (rc) return rc;
    if (!h->owed.scale_pending && !h->owed.kick_pending) return TGNH_OK;
    rc = materialize_chain(h, s); if (rc) return rc;
    if (h->owed.scale_pending) {
        rc = run_tile(h, (h->owed.kick_pending ? OP_PREKICK : 0) | OP_SCALE, KID_SCALE, s, h->thermo.d_state + h->thermo.L.off_scale_a); if (rc) return rc;
        HIP_OK(hipMemcpyAsync(h->thermo.d_state + h->thermo.L.off_scale, h->thermo.d_state + h->thermo.L.off_scale_b, sizeof(double) * h->thermo.L.NT,
                              hipMemcpyDeviceToDevice, s));
    } else {
        rc = run_tile(h, OP_KICK, KID_OTHER, s); if (rc) return rc;
    }
    if (big_com_on(h)) { rc = run_big_com(h, false, s); if (rc) return rc; }   // the velocities just changed: refresh the COM table
    h->owed.velocities_current();      // first_half_done stays
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_flush(tgnh_handle h, void* stream) {
    CHECK_H(h);
    if (!h->owed.scale_pending && !h->owed.kick_pending && !h->owed.end_pending && !h->owed.planes_live) return TGNH_OK;
    tgnh_status rc = entry(h, true); if (rc) return rc;
    return flush_impl(h, (hipStream_t)stream);
}

extern "C" tgnh_status tgnh_note_replayed_steps(tgnh_handle h, int nsteps) {
    CHECK_H(h);
    if (nsteps < 0) return fail(TGNH_ERR_ARG, "negative step count");
    h->run.time += h->d.step_size * nsteps;
    h->run.step_count += nsteps;
    return TGNH_OK;
}

// Restores the clock of a checkpointed run (the reference keeps time / stepCount in the platform data, Ref :413-414,
// Cu :405-406, and OpenMM's checkpoints carry them).
extern "C" tgnh_status tgnh_set_time(tgnh_handle h, double time, int64_t step_count) {
    CHECK_H(h);
    if (step_count < 0) return fail(TGNH_ERR_ARG, "negative step count");
    h->run.time = time;
    h->run.step_count = step_count;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_pending_state(tgnh_handle h, uint32_t* bits) {
    CHECK_H(h);
    if (!bits) return fail(TGNH_ERR_ARG, "null out");
    *bits = h->owed.bits() | (h->run.sweep_reverse ? (uint32_t)tgnh_context::Owed::BIT_SWEEP_REVERSE : 0u);
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_state_changed(tgnh_handle h) {
    CHECK_H(h);
    tgnh_status rc = deferred_guard(h, "tgnh_state_changed");
    if (rc) return rc;
    h->owed.ke_carry = false;              // TRUST_STATE_CHANGED: the next thermostat half step sums the kinetic energies again (Cu :474-488)
    // Velocity planes live here means the call comes between tgnh_step_begin and tgnh_step_end (the guard has passed): what the
    // caller is about to write -- positions, or velm after the flush the contract asks for -- must find velm current and stay.
    // The call has no stream of its own: the one the planes were last written on.  velm's w may be rewritten too: checked again.
    if (h->owed.planes_live) { HIP_OK(hipSetDevice(h->device)); rc = settle_end(h, h->vp.stream); if (rc) return rc; }
    if (h->vp.verdict > 0) h->vp.verdict = 0;
    return TGNH_OK;
}
