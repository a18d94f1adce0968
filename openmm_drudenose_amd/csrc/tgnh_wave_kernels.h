// tgnh_wave_kernels.h -- gfx950 (CDNA4) kernels of the DrudeTGNHIntegrator step over WAVE tiles: wke_kernel (the kinetic-energy passes),
// wstep_kernel (a whole deferred time step in one launch).  The work on one wave tile: tgnh_wave_device.h; the meeting of
// wstep_kernel: tgnh_meet_device.h.  Topologies without wave tiles run the kernels of tgnh_tile_kernels.h.  Part of the translation unit tgnh_kernels.hip:
// holds kernels and non-inline host functions, to be included there and nowhere else.
//
// Reference semantics followed (scychon/openmm_drudeNose):
//   K  = platforms/cuda/src/kernels/drudeTGNH.cu
//   Cu = platforms/cuda/src/CudaDrudeTGNHKernels.cpp
//   Ref= platforms/reference/src/ReferenceDrudeTGNHKernels.cpp
#ifndef TGNH_WAVE_KERNELS_H_
#define TGNH_WAVE_KERNELS_H_
#include "tgnh_wave_device.h"
#include "tgnh_meet_device.h"

namespace tgnh {

// ---------------------------------------------------------------------------
// wke_kernel: the kinetic-energy passes (KE; kick+KE; kick+KE without a velocity store) over WAVE tiles.
//
// What such a pass needs per slot beyond its own velocity is its Drude partner (a lane or so away) and its molecule's
// centre-of-mass velocity.  tile_kernel gets both from an LDS image of a 512-slot tile shared by four wavefronts -- store,
// barrier, one thread per molecule walks its slots (12 of 64 lanes busy, five dependent LDS reads each), barrier, look-ups,
// barrier -- and the work-group issues its next loads only then.  Here a wavefront owns <= 64 consecutive slots that never
// cut a molecule or a pair (tgnh_internal.h) and a PRIVATE 2 KiB LDS image: it stores its velocities and masses (component
// arrays, conflict-free) and every lane sums its OWN molecule from the image, in slot order -- the arithmetic and the order of
// tile_kernel's walk, with all lanes busy and no dependence between wavefronts.  A wavefront's LDS operations are processed
// in order, so nothing waits for a barrier; the next tile's global loads are in flight while this one is worked on, the tile
// bounds in scalar registers two tiles ahead.
// Reference: K :82-113 (COM), :119-133 (relative velocities), :138-200 (bins), :307-365 (the kick); Ref :439-460.
// ---------------------------------------------------------------------------
template <int PREC, int OPS, int GB>
__global__ __launch_bounds__(TBLOCK, TGNH_MINWAVES) void wke_kernel(const TileArgs a) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    constexpr bool DO_KICK = (OPS & OP_KICK) != 0, STORE = DO_KICK && !(OPS & OP_NOSTORE);
    static_assert(GB > 0, "register bins only");
    __shared__ double sred[TBLOCK / 64][GB + 2];
    __shared__ mixed s_img[TBLOCK / 64][4][WAVE_SLOTS];          // per wavefront: x[], y[], z[], mass[]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    mixed* const ix = s_img[wv][0]; mixed* const iy = s_img[wv][1]; mixed* const iz = s_img[wv][2]; mixed* const im = s_img[wv][3];
    const int G = a.num_groups;
    const bool use_com = a.use_com != 0;
    const mixed fscale = (mixed)(0.5 * a.dt / 4294967296.0);     // Cu :295
    mixed4* __restrict__ velm = reinterpret_cast<mixed4*>(a.velm);
    commit_staged(a, tid, TBLOCK);                        // take over the thermostat block an in-kernel chain staged (as tile_kernel)
    double ke_g[GB], ke_com = 0.0, ke_drude = 0.0;
#pragma unroll
    for (int b = 0; b < GB; b++) ke_g[b] = 0.0;
    // tail sum: this launch's number (the tag of its rows), read before anything is handed in
    const unsigned gen0 = a.tail_sum ? __hip_atomic_load(&a.sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;

    // Wave tile of wavefront wv in round r: (r gridDim.x + blockIdx.x) 4 + wv -- a work-group streams 4 consecutive wave
    // tiles.  Everything about WHICH tile is wavefront-uniform (scalar registers, scalar loads): the bounds of the tile after
    // next are fetched while this one is worked on, so the vector loads of the next tile never wait for an index.
    const int nw = a.num_wtiles, stride = (int)gridDim.x * (TBLOCK / 64);
    struct Bounds { int ws, y, n; };        // y = the tile's largest molecule | pattern word << 8 (wave_word)
    auto bounds = [&](const int ww, Bounds& b) {
        const int2* t = a.wave_tile + (a.reverse ? nw - 1 - ww : ww);
        b.ws = t[0].x; b.y = t[0].y; b.n = t[1].x - b.ws;
    };
    auto work = [&](const WaveIn<PREC>& cur, const Bounds& bd) {
        mixed4 v = cur.v;
        const uint32_t m = cur.meta;
        const mixed mass = v.w != 0 ? rcp_(v.w) : (mixed)0;
        if (DO_KICK) {                                                   // A7, per particle (tile_body); w = 0: c = 0, v unchanged
            half_kick<ForceFma>(v.x, v.y, v.z, v.w, fscale, cur.fx, cur.fy, cur.fz);
        }
        if (STORE && lane < bd.n) velm[bd.ws + lane] = v;
        const uint32_t role = m & 3u, g = (m >> 2) & 255u;
        // the wavefront's image (its own LDS operations are processed in order: the reads below see these stores, and the
        // stores of the next tile come after this tile's reads -- the fences only keep the compiler from reordering them)
        ix[lane] = v.x; iy[lane] = v.y; iz[lane] = v.z; im[lane] = mass;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- molecular centre-of-mass velocity (K :86-111): every lane sums its own molecule, in slot order
        mixed cx = 0, cy = 0, cz = 0;
        if (use_com) {
            const int j = (int)((m >> 17) & 63u), n1 = (int)((m >> 23) & 63u);
            const int first = lane - j;
            mixed px = 0, py = 0, pz = 0, pm = 0;
            for (int k = 0; k < (bd.y & 255); k++) {                          // (bd.maxn: the tile's largest molecule, a scalar)
                if (k <= n1) {
                    const mixed um = im[first + k];
                    px += ix[first + k] * um; py += iy[first + k] * um; pz += iz[first + k] * um; pm += um;
                }
            }
            const mixed wq = rcp_(pm);                                   // (a padding lane: pm = 0, unused)
            cx = px * wq; cy = py * wq; cz = pz * wq;
            if (j == 0 && lane < bd.n)                                   // once per molecule: M v_com^2 (K :154)
                ke_com += ((double)cx * cx + (double)cy * cy + (double)cz * cz) * (double)pm;
        }
        // ---- bins (K :138-200 ; Ref :439-460).  Every massive slot adds m |v - v_com|^2 to its group's bin; a pair's
        // two terms together are (m1 + m2) |cm - v_com|^2 + mu |v2 - v1|^2 (K :171-186 splits them that way), so the Drude
        // lane moves the second part, mu |v2 - v1|^2, from the group's bin to the Drude bin: the partner is needed for that
        // difference only
        const double rx = v.x - cx, ry = v.y - cy, rz = v.z - cz;          // (in the velocities' own precision, as tile_body)
        double val = v.w != 0 ? (rx * rx + ry * ry + rz * rz) * (double)mass : 0.0;
        if (role == ROLE_DRUDE) {                                        // one lane per pair
            const int pl = lane + (int)((m >> 10) & 127u) - 64;
            const double dx = ix[pl] - v.x, dy = iy[pl] - v.y, dz = iz[pl] - v.z;
            const double mass1 = mass, mass2 = im[pl];
            const double mu = mass1 * mass2 * rcp_(mass1 + mass2);       // reduced mass = 1/invReducedMass (K :178, :185)
            const double d = (dx * dx + dy * dy + dz * dz) * mu;
            ke_drude += d;
            val -= d;
        }
#pragma unroll
        for (int b = 0; b < GB; b++) ke_g[b] += (g == (uint32_t)b) ? val : 0.0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    int w = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (TBLOCK / 64) + wv);
    Bounds b0{}, b1{}, b2{};
    WaveIn<PREC> A, B;
    PatternWord pw;
    auto load = [&](const Bounds& b, WaveIn<PREC>& in) {
        const bool patterned = pw.of(a, (uint32_t)b.y >> 8, lane);
        wave_load<PREC, OPS>(a, b.ws, b.n, patterned, pw.word, lane, in);
    };
    if (w < nw) { bounds(w, b0); load(b0, A); }
    if (w + stride < nw) bounds(w + stride, b1);
    while (w < nw) {                                                     // two tiles per trip: the register images alternate
        if (w + 2 * stride < nw) bounds(w + 2 * stride, b2);
        if (w + stride < nw) load(b1, B);                                // in flight while A is worked on
        work(A, b0);
        w += stride;
        if (w >= nw) break;
        if (w + 2 * stride < nw) bounds(w + 2 * stride, b0);
        if (w + stride < nw) load(b2, A);
        work(B, b1);
        w += stride;
        b1 = b0; b0 = b2;                                                // (scalar moves)
    }
    // ---- one row of partial sums per work-group: 64-lane sums, one LDS hop, fixed order (ke_reduce's layout)
#pragma unroll
    for (int b = 0; b < GB; b++) ke_g[b] = wave_sum(ke_g[b]);
    ke_com = wave_sum(ke_com);
    ke_drude = wave_sum(ke_drude);
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < GB; b++) sred[wv][b] = ke_g[b];
        sred[wv][GB] = ke_com;
        sred[wv][GB + 1] = ke_drude;
    }
    __syncthreads();
    if (tid < GB + 2) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < TBLOCK / 64; k++) t += sred[k][tid];
        const int b = tid < GB ? tid : G + (tid - GB);                 // thermostat of this thread's sum
        if (tid >= GB || tid < G) {
            if (a.tail_sum) {                                            // a tagged cell: data and "it is there" in one 8-byte store, two per double
                unsigned long long* cell = a.rows + row_word((int)blockIdx.x, 2 * b);
                store_tagged(cell, cell + 64, (unsigned long long)(gen0 + 1u) << 32, t);
            } else a.partials[(size_t)blockIdx.x * (G + 2) + b] = t;
        }
    }
    // ---- tail sum: work-group 0 -- which therefore ends last -- collects every work-group's row in row order (fixed order:
    // reproducible bits) and leaves the sums where the row-sum launch would have.  Only it waits, so the grid need not be
    // resident at once; the polling is bounded (status bit 3, as step_kernel's).
    if (a.tail_sum && blockIdx.x == 0) {
        __shared__ double s_tail[TBLOCK / 64][GB + 2];
        const int NT = G + 2;
        double acc[GB + 2];
#pragma unroll
        for (int b = 0; b < GB + 2; b++) acc[b] = 0.0;
        const bool ok = collect_rows<GB, false, TBLOCK>(a, tid, (int)gridDim.x, NT, (unsigned long long)(gen0 + 1u), acc);
        if (!ok) atomicOr(a.status, 16u);                                // a row never came (bounded polling): status bit 4, the host's failure
#pragma unroll
        for (int b = 0; b < GB + 2; b++) {
            if (b < NT) {
                const double t = wave_sum(acc[b]);
                if (lane == 0) s_tail[wv][b] = t;
            }
        }
        // (the barrier of the hand-over doubles as the vote: incomplete sums are not left where the all-reduce and the chain
        // would take them for kinetic energies -- NaN instead, so that nothing integrates on with a partial sum during the
        // up to 64 steps until the host reads the status word; step_meet withholds its send in the same situation)
        const bool all_ok = __syncthreads_and(ok ? 1 : 0) != 0;
        if (tid < NT) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < TBLOCK / 64; k++) t += s_tail[k][tid];
            a.ke_red[tid] = all_ok ? t : __longlong_as_double(0x7ff8000000000000ll);
        }
        if (tid == 0) a.sync[1] = gen0 + 1u;                             // the next launch's rows carry the next tag
    }
}

// ---------------------------------------------------------------------------
// wstep_kernel: step_kernel's whole deferred time step (STEP_DEFER) over WAVE tiles -- wke_kernel's structure for both passes.
//
// A wavefront owns <= 64 consecutive slots and a private LDS image; nothing in a pass waits for another wavefront.  What that
// buys at shard sizes: a pass without barriers, and for a held tile a second pass that starts from registers.  The one-link
// instantiation takes 110 (single) / 121 (mixed, double) VGPRs = 4 wavefronts per SIMD = two 512-thread work-groups per compute
// unit: 512 work-groups = 262 144 slots are resident at once (tests/test_kernel_resources.py asserts the occupancy) -- at 625 k
// slots a wavefront walks 2.4 tiles forward and back, at 5 M slots 19 -- and for the tile it holds across the meeting: its kicked
// velocities, forces, index word, mass and centre-of-mass velocity are pass 1's, its partner's velocity is still in the
// wavefront's image, its positions were fetched before the meeting.  Same meeting (step_meet), same arithmetic per slot as
// tile_body / wke_kernel, same fixed order of every sum.  Topologies without wave tiles (a molecule longer than a wavefront,
// more than 8 temperature groups) and the other step kinds run step_kernel.
//   pass 1   half kick (unstored) + kinetic-energy sums            (Cu :384-388, :474-488)
//   meet     rows -> work-group 0 -> mailboxes -> both chain halves (Cu :433-652 twice)
//   pass 2   the kick again, rescale, half kick, drift, hard wall   (Cu :351-376 ; K :249-301, :307-365, :435-466, :471-574)
// ---------------------------------------------------------------------------

template <int PREC, int GB, bool MULTI, bool PLANES>
__device__ __forceinline__ void wstep_body(const TileArgs& a) {
    typedef typename Prec<PREC>::mixed mixed;
    static_assert(GB > 0, "register bins only");
    __shared__ double s_scale[MAX_GROUPS + 2];
    __shared__ double s_part[WBLOCK / 64][CHAIN_INLINE_SUM_NT];
    __shared__ double s_x[64 + XCHG_MAX_WORLD * CHAIN_INLINE_SUM_NT];
    __shared__ int s_go;
    __shared__ unsigned s_gen;
    __shared__ unsigned long long s_seq1;
    __shared__ mixed s_img[WBLOCK / 64][7][WAVE_SLOTS];          // per wavefront: velocity x, y, z, mass; position x, y, z (hard wall)
    __shared__ double s_block[256];                              // chains of 2-4 links: the thermostat block as it was at entry
    const int tid = threadIdx.x, lane = tid & 63, G = a.num_groups, NT = G + 2;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool chain_wave = tid < 64;
    const int itg = tid & 63;
    if (a.census) { census(a); return; }                  // residency check at tgnh_create, as step_kernel's
    TileEnv<PREC, GB> e;                                   // the kinetic-energy bins, in the shape ke_reduce takes them
    e.tid = tid; e.G = G; e.smem = nullptr; e.wbins0 = nullptr; e.s_scale = s_scale;
    e.clear_ke();
    WaveStep<PREC, GB, PLANES> ws(a, &e, s_scale, &s_img[wv][0][0], lane);    // the per-tile work (tgnh_wave_device.h)
    typedef WaveBounds Bounds;
    auto bounds = [&](const int ww, Bounds& b) { ws.bounds(ww, b); };
    auto load_vf = [&](const Bounds& b, WStepIn<PREC>& in) { ws.load_vf(b, in); };
    auto load_x = [&](const Bounds& b, WStepIn<PREC>& in) { ws.load_x(b, in); };
    auto prepare = [&](WStepIn<PREC>& t, const Bounds& bd, const bool ke) { ws.template prepare<true>(t, bd, ke); };
    auto finish = [&](WStepIn<PREC>& t, const Bounds& bd) { ws.finish(t, bd); };
    auto wfence = [] { WaveStep<PREC, GB, PLANES>::wfence(); };

    // launch number, exchange number and the thermostat state: read before anything is handed in (step_kernel)
    unsigned gen0 = 0;
    unsigned long long seq0 = 0;
    Chain1Regs creg{};
    if (chain_wave) {
        gen0 = __hip_atomic_load(&a.sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seq0 = __hip_atomic_load(a.chain.x.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (itg < NT && !(MULTI && a.chain.L.C > 1)) creg = chain1_load(a.chain, a.st_in, itg);
    }
    // Chains of 2-4 links: the whole block (<= 256 doubles, checked on the host) goes to LDS now -- work-group 0 advances it in
    // place once it holds every row, and a row leaves only behind the barrier in ke_reduce, which every thread reaches after
    // its load has landed and been stored here.
    if (MULTI && a.chain.L.C > 1 && tid < a.chain.L.total) s_block[tid] = a.st_in[tid];

    const int nw = a.num_wtiles, stride = (int)gridDim.x * (WBLOCK / 64);

    // ---- pass 1: this wavefront's tiles w0, w0 + stride, ...; the next tile's loads in flight while one is worked on
    TRACE(0);
    const int w0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (WBLOCK / 64) + wv);
    const bool have = w0 < nw;                             // (a wavefront beyond the last tile only takes part in the meeting)
    int w = w0;
    // One register image: no tile is loaded ahead of the one being worked on.  What hides a tile's load latency is the other
    // wavefronts of the SIMD -- four of them at this register count (a second image was measured at the same occupancy and
    // bought nothing; it would cost the fourth wavefront today).
    // Tile bounds are scalar loads one tile ahead of their use.
    Bounds b0{}, b1{};
    WStepIn<PREC> cur;
    if (have) {
        bounds(w, b0);
        if (w + stride < nw) bounds(w + stride, b1);
        load_vf(b0, cur);
    }
    while (have) {
#ifdef TGNH_TRACE
        if (w == w0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TRACE(3); }
#endif
        prepare(cur, b0, true);
#ifdef TGNH_TRACE
        if (w == w0) TRACE(4);
#endif
        if (w + stride >= nw) break;
        wfence();                                          // (this tile's image reads are done before the next tile's image is stored)
        w += stride;
        b0 = b1;
        if (w + stride < nw) bounds(w + stride, b1);
        load_vf(b0, cur);
    }
    const int w_last = w;                                  // stays in `cur` (kicked velocities, mass, v_com), its image in LDS
    TRACE(1);
    MeetShared sh{s_scale, s_part, s_x, &s_go, &s_gen, &s_seq1, s_block};
    if (!step_meet<PREC, GB, true, WBLOCK, MULTI>(a, e, gen0, seq0, creg, sh, [&] {
            if (have) {
                load_x(b0, cur);
                if (w_last - stride >= 0) bounds(w_last - stride, b1);        // the way back: known long before it is needed
            }
        })) return;

    // ---- pass 2, backwards from the held tile
    TRACE(9);
    if (have) {
        w = w_last;
        finish(cur, b0);                                   // the held tile: everything but its positions is pass 1's
        TRACE(5);
        while (w - stride >= 0) {
            w -= stride;
            b0 = b1;
            if (w - stride >= 0) bounds(w - stride, b1);
            load_vf(b0, cur); load_x(b0, cur);
            prepare(cur, b0, false);
            finish(cur, b0);
        }
    }
    TRACE(15);
}

// The step with the velocities in velm, and the same step with them in the library's x | y | z planes (TileArgs::vplanes set: every
// wave tile patterned, 1/m from wpat_invm).  Two kernels of one body: each is compiled without the other's loads and stores, and
// wstep_kernel is the code it was before the planes existed.
template <int PREC, int GB, bool MULTI = false>
__global__ __launch_bounds__(WBLOCK) void wstep_kernel(const TileArgs a) { wstep_body<PREC, GB, MULTI, false>(a); }
template <int PREC, int GB, bool MULTI = false>
__global__ __launch_bounds__(WBLOCK) void wstep_planes_kernel(const TileArgs a) { wstep_body<PREC, GB, MULTI, true>(a); }

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <int PREC, int OPS> static tile_fn_t wke_fn_gb(int gb) {
    if (gb <= 1) return wke_kernel<PREC, OPS, 1>;
    if (gb <= 4) return wke_kernel<PREC, OPS, 4>;
    return wke_kernel<PREC, OPS, 8>;
}
template <int PREC> static tile_fn_t wke_fn_ops(int ops, int gb) {
    switch (ops) {
        case OP_KE: return wke_fn_gb<PREC, OP_KE>(gb);
        case OP_KICK | OP_KE: return wke_fn_gb<PREC, OP_KICK | OP_KE>(gb);
        case OP_KICK | OP_KE | OP_NOSTORE: return wke_fn_gb<PREC, OP_KICK | OP_KE | OP_NOSTORE>(gb);
        default: return nullptr;
    }
}
static tile_fn_t wke_fn(int precision, int ops, int gb) {
    if (gb == 0) return nullptr;                          // more than 8 groups: LDS bins, the tile kernel
    return with_precision(precision, [&](auto P) -> tile_fn_t { return wke_fn_ops<decltype(P)::value>(ops, gb); });
}
hipError_t launch_wke(int precision, int ops, int gb, const TileArgs& a, int grid, hipStream_t s) {
    tile_fn_t fn = wke_fn(precision, ops, gb);
    if (!fn) return hipErrorInvalidValue;
    TGNH_LAUNCH(fn, dim3(grid), dim3(TBLOCK), 0, s, a);
    return hipGetLastError();
}
int wke_blocks_per_cu(int precision, int ops, int gb) { return blocks_per_cu(wke_fn(precision, ops, gb), TBLOCK, 0); }

template <int PREC, bool MULTI> static tile_fn_t wstep_fn_gb(int gb, bool planes) {
    // (mixed and double only: in single precision the compiler packs the arithmetic of a float4 that is stored whole otherwise than
    // that of three floats stored apart, and contracts it otherwise -- other bits than the velm form's)
    // Neither a store of the three components as one value nor hiding from the compiler that 1/m is the same for every tile changed that.
    if (planes && PREC == TGNH_PREC_SINGLE) return nullptr;
    constexpr int PLANES_PREC = PREC == TGNH_PREC_SINGLE ? TGNH_PREC_MIXED : PREC;      // (no single-precision instantiation is made)
    if (planes) return gb <= 1 ? wstep_planes_kernel<PLANES_PREC, 1, MULTI>
                     : gb <= 4 ? wstep_planes_kernel<PLANES_PREC, 4, MULTI>
                               : wstep_planes_kernel<PLANES_PREC, 8, MULTI>;
    return gb <= 1 ? wstep_kernel<PREC, 1, MULTI> : gb <= 4 ? wstep_kernel<PREC, 4, MULTI> : wstep_kernel<PREC, 8, MULTI>;
}
static tile_fn_t wstep_fn(int precision, int gb, bool multi, bool planes) {
    if (gb == 0) return nullptr;
    return with_precision(precision, [&](auto P) -> tile_fn_t {
        return multi ? wstep_fn_gb<decltype(P)::value, true>(gb, planes) : wstep_fn_gb<decltype(P)::value, false>(gb, planes);
    });
}
hipError_t launch_wstep(int precision, int gb, bool multi, const TileArgs& a, int grid, hipStream_t s) {
    if (a.vplanes && !a.wpat_invm) return hipErrorInvalidValue;
    tile_fn_t fn = wstep_fn(precision, gb, multi, a.vplanes != nullptr);
    if (!fn) return hipErrorInvalidValue;
    TGNH_LAUNCH(fn, dim3(grid), dim3(WBLOCK), 0, s, a);
    return hipGetLastError();
}
int wstep_blocks_per_cu(int precision, int gb, bool multi, bool planes) { return blocks_per_cu(wstep_fn(precision, gb, multi, planes), WBLOCK, 0); }

}  // namespace tgnh
#endif
