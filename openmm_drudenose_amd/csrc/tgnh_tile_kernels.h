// tgnh_tile_kernels.h -- gfx950 (CDNA4) kernels of the DrudeTGNHIntegrator step over 512-slot tiles: tile_kernel, step_kernel.
//
// Design (DESIGN.md "Kernels"): the whole per-particle part of a thermostat or
// velocity-Verlet half step is ONE streaming pass of `tile_kernel`.  A 256-thread
// work-group (4 wavefronts x 64 lanes) owns a tile of <= 512 consecutive slots whose
// ends never cut a Drude pair or a molecule, loads it with one coalesced 16/32-byte
// access per lane, keeps the velocity image in LDS so the Drude partner and the
// molecular centre of mass are LDS look-ups, and leaves with fp64 per-group kinetic
// energy sums reduced over the 64 lanes (wave_sum) + one LDS hop.  Which of
// {rescale, half kick, drift, hard wall, KE} a launch performs is a compile-time mask,
// so e.g. rescale+kick+drift touches each array once.  The Nose-Hoover chains run
// on the device (chain_kernel, fp64), so a step has no host round trip.
// The work on one tile: tgnh_tile_device.h; the meeting of step_kernel: tgnh_meet_device.h; the chain: tgnh_chain_device.h.  The
// same passes over wave tiles (a wavefront's 64 slots): tgnh_wave_kernels.h.  What these tiles cannot hold -- a Drude particle
// more than a tile from its parent, more than 32 temperature groups, residues in several runs -- steps through the reference's
// own un-fused kernels by global index instead: tgnh_gather.hip.  Part of the translation unit tgnh_kernels.hip:
// holds kernels and non-inline host functions, to be included there and nowhere else.
//
// Reference semantics followed (scychon/openmm_drudeNose):
//   K  = platforms/cuda/src/kernels/drudeTGNH.cu
//   Cu = platforms/cuda/src/CudaDrudeTGNHKernels.cpp
//   Ref= platforms/reference/src/ReferenceDrudeTGNHKernels.cpp
#ifndef TGNH_TILE_KERNELS_H_
#define TGNH_TILE_KERNELS_H_
#include "tgnh_tile_device.h"
#include "tgnh_meet_device.h"

namespace tgnh {

size_t tile_lds_bytes(int precision, int ops, bool hardwall, bool use_com) {
    (void)use_com;
    const size_t m4 = (precision == TGNH_PREC_SINGLE) ? 16 : 32;
    const bool hw = hardwall && (ops & (OP_DRIFT | OP_MOVE));
    size_t b = (size_t)(TBLOCK / 64) * (MAX_GROUPS + 2) * 8;          // KE reduction scratch
    if ((ops & (OP_SCALE | OP_KE)) || hw) b = m4 * (TILE_SLOTS + TILE_RES);   // sv + scom (fixed carve)
    if (hw) b += m4 * TILE_SLOTS;                                     // sx
    return b;
}

// ---------------------------------------------------------------------------
// tile_kernel
// ---------------------------------------------------------------------------

// MULTI: the in-kernel chain may have 2-4 links (chainN_run: ~100 registers of its own).  Its own instantiation, so that the
// one-link kernels keep their register count; and in it no wavefront issues its first tile's loads before the chain is done --
// the image of a tile in flight and the chain's links together would not fit three work-groups per compute unit.
template <int PREC, int OPS, int GB, bool MULTI = false>
__global__ __launch_bounds__(TBLOCK, TGNH_MINWAVES) void tile_kernel(const TileArgs a) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef OpsOf<OPS> O;
    constexpr bool DO_SCALE = O::DO_SCALE, DO_KE = O::DO_KE, POS = O::POS;

    __shared__ double s_scale[MAX_GROUPS + 2];           // velocity scale factors of this launch (80 B: keeps smem 16-B aligned)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int G = a.num_groups;
    TileEnv<PREC, GB> e;
    e.init(a, smem, s_scale, POS && a.hardwall != 0);
    TilePattern tp;
    auto load_tile = [&](int tt, TileIn<PREC>& in) { tile_load<PREC, OPS, 0, OpsOf<OPS>::POS || OpsOf<OPS>::VEL_W>(a, a.reverse ? a.num_tiles - 1 - tt : tt, in, tp); };

    TileIn<PREC> cur;
    TRACE(0);
    commit_staged(a, tid, TBLOCK);                        // take over the thermostat block an in-kernel chain staged
    // ---- scale factors.  With a one-link chain the Nose-Hoover update itself runs here (A5): every work-group
    // computes the same factors from the same summed kinetic energies (fp64, deterministic); work-group 0 alone
    // writes the advanced thermostat block -- to a staging copy, because work-groups of this launch may start after
    // work-group 0 has finished.  One wavefront per work-group runs the chain, and runs it BEFORE issuing its own
    // tile loads: behind them, its wait for the thermostat state would be a wait for the whole tile (the counter
    // of outstanding loads completes in order), and every wavefront of the work-group would stand at the barrier
    // below for the latency of the memory phase PLUS the chain.  This way the chain (~3.5 us) hides behind the other
    // three wavefronts' loads.  (Wavefront 0 everywhere: the dispatcher starts consecutive work-groups of a compute
    // unit on consecutive SIMDs -- HW_ID, tools/trace_probe.py -- so the resident chains already sit on different
    // SIMDs; rotating the wavefront by residency slot made two of three collide.)
    const bool chain_wave = DO_SCALE && a.chain_on && tid < 64;
    const bool have_tile = (int)blockIdx.x < a.num_tiles;
    // sum_rows == 2 (many partial rows, no chain launch): ALL four wavefronts read a quarter of the rows each, in
    // batches of 16 loads issued ahead of the tile loads, so the row read costs one or two memory latencies that the
    // tile loads overlap -- read by the chain wavefront alone it was a chain of L2 misses on the critical path.
    // Flat view of the rows as in chain_sum_rows: lane l < W of wavefront w starts at element w W + l, stride 4 W.
    double racc = 0.0;
    int rcol = -1;
    __shared__ double s_part[TBLOCK / 64][CHAIN_INLINE_SUM_NT];
    if (DO_SCALE && a.chain_on && a.sum_rows == 2) {
        const int NT = G + 2, W = 64 - 64 % NT, lane = tid & 63;
        if (lane < W) {
            rcol = lane % NT;
            const int n = a.chain.nparts * NT, stride = (TBLOCK / 64) * W;
            for (int f0 = (tid >> 6) * W + lane; f0 < n; f0 += 16 * stride) {
                double v[16];
#pragma unroll
                for (int k = 0; k < 16; k++) { const int f = f0 + k * stride; v[k] = f < n ? a.chain.partials[f] : 0.0; }
#pragma unroll
                for (int k = 0; k < 16; k++) racc += v[k];
            }
            const double* big = a.chain.partials + (size_t)GRID_CAP * NT;
            for (int f = (tid >> 6) * W + lane; f < a.chain.nbig * NT; f += stride) racc += big[f];
        }
    }
    if (!MULTI && !chain_wave && have_tile) load_tile(blockIdx.x, cur);
    if (DO_SCALE && a.chain_on && a.sum_rows == 2) {
        const int NT = G + 2;
        for (int b = 0; b < NT; b++) {
            const double tb = wave_sum(rcol == b ? racc : 0.0);
            if ((tid & 63) == 0) s_part[tid >> 6][b] = tb;
        }
        __syncthreads();
    }
    TRACE(1);
    int trace_tile = 0; (void)trace_tile;
#ifdef TGNH_TRACE
    if ((threadIdx.x & 63) == 0) {          // slots 11/12: where the hardware put wavefronts 0 and 1 (HW_ID, XCC_ID)
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        if (threadIdx.x == 0) g_trace[blockIdx.x * 16 + 11] = ((unsigned long long)xcc << 32) | hw;
        if (threadIdx.x == 64) g_trace[blockIdx.x * 16 + 12] = ((unsigned long long)xcc << 32) | hw;
    }
#endif
    if (DO_SCALE) {
        const int NT = G + 2;
        if (a.chain_on) {
            if (chain_wave) {
                const ChainLayout& L = a.chain.L;
                const bool write = blockIdx.x == 0;
                const int itg = tid & 63;
                TRACE(13);
                const bool one_link = !MULTI || L.C == 1;            // (2-4 links: chainN_run reads its state itself)
                Chain1Regs creg{};
                if (itg < NT) { if (one_link) creg = chain1_load(a.chain, a.st_in, itg); else creg.ke = a.st_in[chain_ke_src(a.chain) + itg]; }
                if (a.x_wait) {                                      // sharded: everybody's sums arrive by mailbox
                    const double tot = xchg_wait_sum(a.chain.x, NT, itg, reinterpret_cast<double*>(smem));   // the images are not in use yet
                    creg.ke = tot;
                    if (itg < NT) s_scale[itg] = tot;                // parked for the KESum below (same wavefront: in order)
                    if (write && itg < NT) a.chain.st[L.off_ke_red + itg] = tot;   // nobody reads it there in this launch
                }
                if (a.sum_rows) {                                    // no chain launch: the rows are summed in this launch
                    double mine = 0.0, ks = 0.0;
                    if (a.sum_rows == 2) {                           // the four wavefronts' quarters, in wavefront order
                        for (int b = 0; b < NT; b++) {
                            double tb = 0.0;
#pragma unroll
                            for (int w = 0; w < TBLOCK / 64; w++) tb += s_part[w][b];
                            mine = itg == b ? tb : mine;
                            ks += tb;
                        }
                    } else {
                        chain_sum_rows(a.chain, itg, &mine, &ks);      // a handful of rows: this wavefront alone
                    }
                    creg.ke = mine;
                    if (write && itg < NT) a.chain.st[L.off_ke_red + itg] = mine;   // nobody reads it there in this launch
                    if (write && itg == 63) a.st_out[L.off_kesum] = 0.5 * ks;       // Cu :493-497
                } else if (write && itg == 63) {                     // Cu :493-497
                    double s = 0.0;
                    for (int i = 0; i < NT; i++) s += a.x_wait ? s_scale[i] : a.st_in[chain_ke_src(a.chain) + i];
                    a.st_out[L.off_kesum] = 0.5 * s;
                }
                if (write && itg < NT && !a.chain.ke_carry && creg.ke != creg.ke) atomicOr(a.status, 16u);     // a NaN sum (a tail sum that gave up, here or on a peer rank): chain_prologue's check
                if (MULTI && !one_link) chainN_run(a.chain, a.st_in, a.st_out, write, s_scale, itg, creg.ke);
                else if (itg < NT) {
                    if (L.c1_quirk) chain1q_run(a.chain, creg, a.st_out, write, s_scale, itg);
                    else chain1_run(a.chain, creg, a.st_out, write, s_scale, itg);
                }
                TRACE(14);
                if (have_tile) load_tile(blockIdx.x, cur);
            } else if (MULTI && have_tile) load_tile(blockIdx.x, cur);
        } else {
            if (tid < NT) s_scale[tid] = a.scale[tid];
            if (MULTI && have_tile) load_tile(blockIdx.x, cur);
        }
        __syncthreads();
        e.s_com = (mixed)s_scale[G]; e.s_drude = (mixed)s_scale[G + 1];
    }
    TRACE(2);
    for (int t = blockIdx.x; t < a.num_tiles; t += gridDim.x) {
        const bool more = t + (int)gridDim.x < a.num_tiles;
        tile_body<PREC, OPS, GB>(a, e, cur, trace_tile);
        TRACE(6 + 4 * trace_tile);
#ifdef TGNH_TRACE
        trace_tile++;
#endif
        if (more) load_tile(t + gridDim.x, cur);
    }
    if (DO_KE) ke_reduce<PREC, GB, false>(a, e);
    TRACE(15);
}

// ---------------------------------------------------------------------------
// step_kernel: a whole time step of the deferred pass structure in ONE launch (TGNH_FLAG_RESIDENT_STEP).
//
//   pass 1   half kick (unstored) + kinetic-energy sums over the work-group's tiles          (Cu :384-388, :474-488)
//   meet     every work-group leaves its row of sums as tagged cells (data and "it is there" in one 8-byte store);
//            work-group 0 collects the rows (fixed order: reproducible bits), and sends the sums to the mailbox of
//            every rank -- its own included; unsharded, the handle's private one-rank mailbox -- where every
//            work-group of every rank waits for all ranks' sums.  No read-modify-write atomics anywhere: 768
//            work-groups arriving at one counter cost ~70 us, plain tagged stores and polling loads a few
//   chain    both thermostat half steps back to back, by one wavefront of every work-group      (Cu :433-652 twice)
//   pass 2   the kick again, rescale, half kick, drift, hard wall over the same tiles           (Cu :351-376)
//
// The grid is the work-groups that are resident at once (occupancy x CUs), so work-group 0's wait cannot deadlock as
// long as this launch has its share of the device to itself; every wait is bounded all the same (status bits 2 / 3,
// never a hung device).  Pass 2 walks the work-group's tiles backwards: its first tile is pass 1's last, whose
// velocities, forces and index words are still in registers -- only its positions are fetched, and that before the
// meeting, which hides them.  At shard sizes (<= 2 tiles per work-group) most of the step's state therefore never
// leaves the chip between the passes.  The thermostat block is advanced in place by work-group 0: every work-group
// reads it before it hands in its row, and work-group 0 writes only after it has everybody's.
// ---------------------------------------------------------------------------
// The two passes are template parameters, so the same kernel also runs the thermostat halves of the reference's own pass
// structure (velocities never lag: what the OpenMM glue may use) as one launch each:
//   STEP_DEFER        kick+KE (unstored)  |  kick again, rescale, kick, drift     both chain halves   a whole deferred step
//   STEP_PLAIN_BEGIN  KE                  |  rescale, kick, drift                 one half            Cu :336-376
//   STEP_PLAIN_END    kick+KE (unstored)  |  kick again, rescale                  one half            Cu :384-402
//   STEP_SPLIT_BEGIN  KE                  |  rescale, kick, posDelta              one half            Cu :336-360 (constraints)
//   STEP_SPLIT_END    KE                  |  rescale                              one half            Cu :394-402 (constraints)
enum : int { STEP_DEFER = 0, STEP_PLAIN_BEGIN = 1, STEP_PLAIN_END = 2, STEP_SPLIT_BEGIN = 3, STEP_SPLIT_END = 4, STEP_KINDS = 5 };
constexpr int step_ops1(int kind) {
    return (kind == STEP_DEFER || kind == STEP_PLAIN_END) ? (OP_KICK | OP_KE | OP_NOSTORE) : OP_KE;
}
constexpr int step_ops2(int kind) {
    return kind == STEP_DEFER ? (OP_PREKICK | OP_SCALE | OP_KICK | OP_DRIFT)
         : kind == STEP_PLAIN_BEGIN ? (OP_SCALE | OP_KICK | OP_DRIFT)
         : kind == STEP_PLAIN_END ? (OP_PREKICK | OP_SCALE)
         : kind == STEP_SPLIT_BEGIN ? (OP_SCALE | OP_KICK | OP_POSDELTA)
         : OP_SCALE;
}

// (Measured and dropped, profiles/r02_resident_tuning.md: a second register image to load a work-group's next tile under
// the current one -- in both passes: 198 VGPRs, occupancy 2; in pass 1 alone: free in registers, no gain -- and tiles cut
// to N / (k x work-groups) slots for equal walks.  A pass costs ~2 us of a compute unit's time per tile whether a
// work-group walks one tile or two: it is the unit's three resident work-groups that overlap each other, not a
// work-group its own tiles.  Pass 2 already moves its 73 MB at the 6.6 TB/s the Infinity Cache gives.)
template <int PREC, int GB, int KIND>
__global__ __launch_bounds__(TBLOCK, TGNH_MINWAVES) void step_kernel(const TileArgs a) {
    typedef typename Prec<PREC>::mixed mixed;
    constexpr int STEP_OPS1 = step_ops1(KIND), STEP_OPS2 = step_ops2(KIND);
    __shared__ double s_scale[MAX_GROUPS + 2];
    __shared__ double s_part[TBLOCK / 64][CHAIN_INLINE_SUM_NT];
    __shared__ double s_x[64 + XCHG_MAX_WORLD * CHAIN_INLINE_SUM_NT];      // scratch of the sums and the exchange: the images stay intact
    __shared__ int s_go;
    __shared__ unsigned s_gen;
    __shared__ unsigned long long s_seq1;                  // the number of the exchange this launch sends and waits for
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, G = a.num_groups, NT = G + 2;
    const int grid = (int)gridDim.x;
    const bool chain_wave = tid < 64;
    const int itg = tid & 63;
    if (a.census) { census(a); return; }                  // the residency check at tgnh_create: nothing else is touched
    TileEnv<PREC, GB> e;
    e.init(a, smem, s_scale, OpsOf<STEP_OPS2>::POS && a.hardwall != 0);
    auto tile_of = [&](int tt) { return a.reverse ? a.num_tiles - 1 - tt : tt; };

    // this launch's number (the tag of its rows), the exchange it will wait for and this wavefront's thermostat state: read
    // before anything is handed in.  The thermostat block is advanced IN PLACE by work-group 0 once it holds every row, so
    // every work-group must have READ the block before its row goes out: the loads are issued here, ahead of the first
    // tile's (loads return in order), and their registers are pinned just before ke_reduce's tagged stores below, which the
    // same wavefront issues -- the order is program order plus a data dependency, not a matter of latencies.
    unsigned gen0 = 0;
    unsigned long long seq0 = 0;
    Chain1Regs creg{};
    if (chain_wave) {
        gen0 = __hip_atomic_load(&a.sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seq0 = __hip_atomic_load(a.chain.x.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (itg < NT) creg = chain1_load(a.chain, a.st_in, itg);
    }

    // ---- pass 1
    TRACE(0);
    TileIn<PREC> cur;
    int tt = blockIdx.x;                                   // grid <= num_tiles: every work-group has a tile
    TilePattern tp;
    tile_load<PREC, STEP_OPS1>(a, tile_of(tt), cur, tp);
    for (;;) {
        tile_body<PREC, STEP_OPS1, GB>(a, e, cur, 4);      // (trace slots >= 16: not recorded)
        if (tt + grid >= a.num_tiles) break;
        tt += grid;
        tile_load<PREC, STEP_OPS1>(a, tile_of(tt), cur, tp);
    }
    const int tt_last = tt;                                // stays in `cur`; its velocity image and COM table stay in LDS
    TRACE(1);
    MeetShared sh{s_scale, s_part, s_x, &s_go, &s_gen, &s_seq1, nullptr};
    if (!step_meet<PREC, GB>(a, e, gen0, seq0, creg, sh, [&] { tile_load<PREC, STEP_OPS2, STEP_OPS1>(a, tile_of(tt_last), cur, tp); }))
        return;                                            // an exchange timed out: reported by the status word; nothing is stored
    e.s_com = (mixed)s_scale[G]; e.s_drude = (mixed)s_scale[G + 1];
    TRACE(9);

    // ---- pass 2, backwards from the held tile
    tt = tt_last;
    for (bool held = true;; held = false) {                // (one call site: two cost 40 VGPRs and a work-group per CU)
        tile_body<PREC, STEP_OPS2, GB>(a, e, cur, 0, held);  // the held tile: image and COM table of pass 1
        if (tt - grid < 0) break;
        tt -= grid;
        tile_load<PREC, STEP_OPS2>(a, tile_of(tt), cur, tp);
    }
    TRACE(15);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

template <int PREC, int OPS>
static tile_fn_t tile_fn_gb(int gb) {
    if constexpr ((OPS & OP_KE) != 0) {
        if (gb == 0) return tile_kernel<PREC, OPS, 0>;
        if (gb <= 1) return tile_kernel<PREC, OPS, 1>;
        if (gb <= 4) return tile_kernel<PREC, OPS, 4>;
        return tile_kernel<PREC, OPS, 8>;
    } else {
        return tile_kernel<PREC, OPS, 1>;
    }
}

template <int PREC>
static tile_fn_t tile_fn_ops(int ops, int gb) {
    switch (ops) {
        case OP_KE: return tile_fn_gb<PREC, OP_KE>(gb);
        case OP_SCALE: return tile_fn_gb<PREC, OP_SCALE>(gb);
        case OP_SCALE | OP_KICK | OP_DRIFT: return tile_fn_gb<PREC, OP_SCALE | OP_KICK | OP_DRIFT>(gb);
        case OP_KICK | OP_KE: return tile_fn_gb<PREC, OP_KICK | OP_KE>(gb);
        case OP_KICK | OP_KE | OP_NOSTORE: return tile_fn_gb<PREC, OP_KICK | OP_KE | OP_NOSTORE>(gb);
        case OP_PREKICK | OP_SCALE | OP_KICK | OP_DRIFT: return tile_fn_gb<PREC, OP_PREKICK | OP_SCALE | OP_KICK | OP_DRIFT>(gb);
        case OP_PREKICK | OP_SCALE: return tile_fn_gb<PREC, OP_PREKICK | OP_SCALE>(gb);
        case OP_KICK: return tile_fn_gb<PREC, OP_KICK>(gb);
        case OP_SCALE | OP_KICK | OP_POSDELTA: return tile_fn_gb<PREC, OP_SCALE | OP_KICK | OP_POSDELTA>(gb);
        case OP_MOVE: return tile_fn_gb<PREC, OP_MOVE>(gb);
        default: return nullptr;
    }
}

static tile_fn_t tile_fn(int precision, int ops, int gb) {
    return with_precision(precision, [&](auto P) -> tile_fn_t { return tile_fn_ops<decltype(P)::value>(ops, gb); });
}

// the instantiations whose in-kernel chain may have 2-4 links (rescale launches only; no KE bins in any of them)
template <int PREC> static tile_fn_t tile_fn_multi(int ops) {
    switch (ops) {
        case OP_SCALE: return tile_kernel<PREC, OP_SCALE, 1, true>;
        case OP_SCALE | OP_KICK | OP_DRIFT: return tile_kernel<PREC, OP_SCALE | OP_KICK | OP_DRIFT, 1, true>;
        case OP_PREKICK | OP_SCALE | OP_KICK | OP_DRIFT: return tile_kernel<PREC, OP_PREKICK | OP_SCALE | OP_KICK | OP_DRIFT, 1, true>;
        case OP_PREKICK | OP_SCALE: return tile_kernel<PREC, OP_PREKICK | OP_SCALE, 1, true>;
        case OP_SCALE | OP_KICK | OP_POSDELTA: return tile_kernel<PREC, OP_SCALE | OP_KICK | OP_POSDELTA, 1, true>;
        default: return nullptr;
    }
}
static tile_fn_t tile_fn_any(int precision, int ops, int gb, bool multi) {
    if (!multi) return tile_fn(precision, ops, gb);
    return with_precision(precision, [&](auto P) -> tile_fn_t { return tile_fn_multi<decltype(P)::value>(ops); });
}

hipError_t launch_tile(int precision, int ops, int gb, const TileArgs& a, int grid, size_t lds, hipStream_t s) {
    tile_fn_t fn = tile_fn_any(precision, ops, gb, a.chain_on && a.chain.L.C > 1);
    if (!fn) return hipErrorInvalidValue;
    TGNH_LAUNCH(fn, dim3(grid), dim3(TBLOCK), lds, s, a);
    return hipGetLastError();
}

template <int PREC, int KIND> static tile_fn_t step_fn_gb(int gb) {
    if (gb <= 1) return step_kernel<PREC, 1, KIND>;
    if (gb <= 4) return step_kernel<PREC, 4, KIND>;
    return step_kernel<PREC, 8, KIND>;
}
template <int PREC> static tile_fn_t step_fn_kind(int kind, int gb) {
    switch (kind) {
        case STEP_DEFER: return step_fn_gb<PREC, STEP_DEFER>(gb);
        case STEP_PLAIN_BEGIN: return step_fn_gb<PREC, STEP_PLAIN_BEGIN>(gb);
        case STEP_PLAIN_END: return step_fn_gb<PREC, STEP_PLAIN_END>(gb);
        case STEP_SPLIT_BEGIN: return step_fn_gb<PREC, STEP_SPLIT_BEGIN>(gb);
        case STEP_SPLIT_END: return step_fn_gb<PREC, STEP_SPLIT_END>(gb);
        default: return nullptr;
    }
}
static tile_fn_t step_fn(int precision, int gb, int kind) {
    if (gb == 0) return nullptr;                          // more than 8 groups: the tile kernels
    return with_precision(precision, [&](auto P) -> tile_fn_t { return step_fn_kind<decltype(P)::value>(kind, gb); });
}
int step_kind_ops2(int kind) { return step_ops2(kind); }
hipError_t launch_step(int precision, int gb, int kind, const TileArgs& a, int grid, size_t lds, hipStream_t s) {
    tile_fn_t fn = step_fn(precision, gb, kind);
    if (!fn) return hipErrorInvalidValue;
    TGNH_LAUNCH(fn, dim3(grid), dim3(TBLOCK), lds, s, a);
    return hipGetLastError();
}
int step_blocks_per_cu(int precision, int gb, int kind, size_t lds) { return blocks_per_cu(step_fn(precision, gb, kind), TBLOCK, lds); }
int tile_blocks_per_cu(int precision, int ops, int gb, size_t lds, bool multi) { return blocks_per_cu(tile_fn_any(precision, ops, gb, multi), TBLOCK, lds); }

}  // namespace tgnh
#endif
