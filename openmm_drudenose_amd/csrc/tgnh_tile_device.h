// tgnh_tile_device.h -- device code of the 512-slot tiles (tile_kernel, step_kernel: tgnh_tile_kernels.h): the LDS carve and the
// kinetic-energy bins of a work-group (TileEnv; the wave-tile step kernel keeps its bins in the same shape) with their work-group
// reduction, a tile's global loads and the work on one tile (tile_body).  Included by .hip files only.
// Reference semantics followed (scychon/openmm_drudeNose):
//   K  = platforms/cuda/src/kernels/drudeTGNH.cu
//   Cu = platforms/cuda/src/CudaDrudeTGNHKernels.cpp
//   Ref= platforms/reference/src/ReferenceDrudeTGNHKernels.cpp
#ifndef TGNH_TILE_DEVICE_H_
#define TGNH_TILE_DEVICE_H_
#include "tgnh_device_math.h"
#include "tgnh_trace.h"
#include "tgnh_xchg_device.h"
#include "tgnh_slot_device.h"

namespace tgnh {

#ifndef TGNH_MINWAVES
#define TGNH_MINWAVES 1
#endif

// What a work-group carries through a launch: the LDS carve, its KE accumulators, launch constants.
template <int PREC, int GB> struct TileEnv {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    // fp64 images are kept component-wise (x[], y[], z[], w[]): a 32-byte double4 per lane is a 2-way bank conflict on
    // every ds_read/ds_write_b128 and on the per-molecule walk (SQ_LDS_BANK_CONFLICT was 48 % of the LDS cycles);
    // 8-byte components at lane stride 8 (or 8 x molecule size) are conflict-free.  float4 images stay packed.
    static constexpr bool SOA = sizeof(mixed) == 8;
    static constexpr int GBR = GB > 0 ? GB : 1;
    mixed4* sv;              // [TILE_SLOTS] velocity image
    mixed4* scom;            // [TILE_RES]   molecular COM velocity, w = 1/M
    mixed4* sx;              // [TILE_SLOTS] position image (hard wall only)
    double* s_scale;         // [NT] velocity scale factors of this launch
    double* wbins0;          // more than 8 groups: one row of fp64 bins per wavefront in LDS, behind the images (GB == 0)
    char* smem;
    int tid, G;
    bool use_com;
    mixed dt, fscale, s_com, s_drude;
    double ke_g[GBR], ke_com, ke_drude;
    __device__ __forceinline__ static void st_img(mixed4* img, int i, const mixed4& u) {
        mixed* imgc = reinterpret_cast<mixed*>(img);
        if (SOA) { imgc[i] = u.x; imgc[TILE_SLOTS + i] = u.y; imgc[2 * TILE_SLOTS + i] = u.z; imgc[3 * TILE_SLOTS + i] = u.w; }
        else img[i] = u;
    }
    __device__ __forceinline__ static mixed4 ld_img(const mixed4* img, int i) {
        const mixed* imgc = reinterpret_cast<const mixed*>(img);
        if (SOA) return mk4(imgc[i], imgc[TILE_SLOTS + i], imgc[2 * TILE_SLOTS + i], imgc[3 * TILE_SLOTS + i]);
        return img[i];
    }
    __device__ __forceinline__ void init(const TileArgs& a, char* smem_, double* s_scale_, bool hardwall_lds) {
        smem = smem_; s_scale = s_scale_;
        sv = reinterpret_cast<mixed4*>(smem); scom = sv + TILE_SLOTS; sx = scom + TILE_RES;
        tid = threadIdx.x; G = a.num_groups; use_com = a.use_com != 0;
        dt = (mixed)a.dt;
        fscale = (mixed)(0.5 * a.dt / 4294967296.0);     // Cu :295
        s_com = 1; s_drude = 1;
        wbins0 = reinterpret_cast<double*>(sx + (hardwall_lds ? TILE_SLOTS : 0));
        clear_ke();
    }
    __device__ __forceinline__ void clear_ke() {
#pragma unroll
        for (int b = 0; b < GBR; b++) ke_g[b] = 0.0;
        ke_com = 0.0; ke_drude = 0.0;
        if (GB == 0) { double* w = wbins0 + (tid >> 6) * G; for (int g = tid & 63; g < G; g += 64) w[g] = 0.0; }
    }
};

// Work-group reduction of the fp64 KE bins: 64-lane sums (wave_sum), then one LDS hop; one row of `partials` per work-group.
// TAGGED: the row is read by another work-group of the SAME launch (step_kernel): every sum goes out as a cell of two
// 8-byte words {32 bits of the double, tag} into a.rows -- data and "it is there" in one atomic store, as in the mailboxes.
template <int PREC, int GB, bool TAGGED, int NTH = TBLOCK>
__device__ __forceinline__ void ke_reduce(const TileArgs& a, TileEnv<PREC, GB>& e, const unsigned tag = 0u, double* scratch = nullptr) {
    typedef TileEnv<PREC, GB> E;
    const int tid = e.tid, G = e.G;
    double (&ke_g)[E::GBR] = e.ke_g;
    double ke_com = e.ke_com, ke_drude = e.ke_drude;
    // thermostat b of this work-group's row (tagged rows: row_word's layout)
    auto put = [&](const int b, double v) {
        if (TAGGED) {
            unsigned long long* cell = a.rows + row_word((int)blockIdx.x, 2 * b);
            store_tagged(cell, cell + 64, (unsigned long long)tag << 32, v);
        } else a.partials[(size_t)blockIdx.x * (G + 2) + b] = v;
    };
    double* sred = scratch ? scratch : reinterpret_cast<double*>(e.smem);   // [TBLOCK/64][GB+2]
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int b = 0; b < GB; b++) ke_g[b] = wave_sum(ke_g[b]);
    if (GB == 0) __syncthreads();                                // every wave's LDS bins are final
    ke_com = wave_sum(ke_com);
    ke_drude = wave_sum(ke_drude);
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < GB; b++) sred[wv * (GB + 2) + b] = ke_g[b];
        sred[wv * (GB + 2) + GB] = ke_com;
        sred[wv * (GB + 2) + GB + 1] = ke_drude;
    }
    __syncthreads();
    if (tid < GB + 2) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NTH / 64; w++) s += sred[w * (GB + 2) + tid];   // fixed order
        if (tid < GB) { if (tid < G) put(tid, s); }
        else put(G + (tid - GB), s);
    }
    if (GB == 0) {
        const double* w0 = e.wbins0;
        for (int g = tid; g < G; g += NTH) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < NTH / 64; w++) s += w0[w * G + g];     // fixed order
            put(g, s);
        }
    }
}

// Raw register image of one tile's global loads.
template <int PREC> struct TileIn {
    int ts, te, rs, nres;
    typename Prec<PREC>::mixed4 v[SPT];
    uint32_t meta[SPT];
    long long fx[SPT], fy[SPT], fz[SPT];
    typename Prec<PREC>::real4 p[SPT];
    float4 c[SPT];
    typename Prec<PREC>::mixed4 pd[SPT];
    int2 rt;                 // this lane's molecule entry (lane r < nres): fetched with the tile, not after the first barrier
};

// Tiles of identical molecules (PATTERN_WORDS, tgnh_internal.h): a thread's slots sit at the same positions in every tile, so the
// words it forms for one tile of a pattern are the words of the next -- kept in registers, formed again when the pattern changes
// (a water box: once per launch; the pattern's lines would otherwise be fetched by every wavefront of the chip for every tile).
struct TilePattern {
    uint32_t pat = 0u;
    uint32_t word[SPT] = {};
};

// which arrays a pass touches
template <int OPS> struct OpsOf {
    static constexpr bool DO_SCALE = OPS & OP_SCALE, DO_KICK = OPS & OP_KICK, DO_DRIFT = OPS & OP_DRIFT;
    static constexpr bool DO_KE = OPS & OP_KE, DO_PD = OPS & OP_POSDELTA, DO_MOVE = OPS & OP_MOVE;
    // OP_PREKICK: the half kick a kick+KE pass of the previous step formed for its sums but did not store
    // (OP_NOSTORE) is applied first -- same force buffer, same expression, same bits (DESIGN.md "deferred kick")
    static constexpr bool DO_PREKICK = OPS & OP_PREKICK, NOSTORE = OPS & OP_NOSTORE;
    static constexpr bool NEED_F = DO_KICK || DO_PREKICK;
    static constexpr bool POS = DO_DRIFT || DO_MOVE;            // positions are read and written
    static constexpr bool VEL_W = (DO_SCALE || DO_KICK || DO_MOVE) && !NOSTORE;   // velocities are written
};

// issue the global loads of tile t for a pass with operations OPS.  HAVE != 0: `in` already holds what a pass with
// operations HAVE loaded for this very tile (velocities, index words, and its forces if it needed them): fetch the rest.
// PATTERN = false: always the per-slot words (tile_kernel's read-only KE passes, at their register budget of 5 work-groups per CU).
template <int PREC, int OPS, int HAVE = 0, bool PATTERN = true>
__device__ __forceinline__ void tile_load(const TileArgs& a, const int t, TileIn<PREC>& in, TilePattern& tp) {
    constexpr bool KEEP_VF = HAVE != 0;
    constexpr bool LOAD_F = OpsOf<OPS>::NEED_F && !(KEEP_VF && OpsOf<HAVE>::NEED_F);
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::real4 real4;
    typedef typename Prec<PREC>::mixed4 mixed4;
    typedef OpsOf<OPS> O;
    const int tid = threadIdx.x;
    const mixed4* __restrict__ velm = reinterpret_cast<const mixed4*>(a.velm);
    const real4* __restrict__ posq = reinterpret_cast<const real4*>(a.posq);
    const float4* __restrict__ pcorr = reinterpret_cast<const float4*>(a.posq_corr);
    const mixed4* __restrict__ pdelta = reinterpret_cast<const mixed4*>(a.pos_delta);
    if (!KEEP_VF) {
        in.ts = a.tile_start[t]; in.te = a.tile_start[t + 1];
        in.rs = a.tile_res[t]; in.nres = a.tile_res[t + 1] - in.rs;
        if ((O::DO_SCALE || O::DO_KE) && a.use_com && tid < in.nres) in.rt = a.res_table[in.rs + tid];
    }
    // a tile of identical molecules: the slot's word from its position (TilePattern), no 4 B per slot from HBM
    const uint32_t pat = (KEEP_VF || !PATTERN) ? 0u : a.tile_pat[t];
    if (pat != 0u && pat != tp.pat) {                             // (work-group-uniform)
        const int period = (int)(pat & 255u), mols = (int)((pat >> 8) & 255u);
        const uint32_t* __restrict__ words = a.pattern + (size_t)(pat >> 16) * PATTERN_WORDS;
        const float rperiod = __builtin_amdgcn_rcpf((float)period);
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            const int pos = k * TBLOCK + tid;
            const int q = (int)(((float)pos + 0.5f) * rperiod);          // pos div period (pos < 512, period <= 64: never within rounding of an integer)
            tp.word[k] = words[pos - q * period] + (a.use_com ? (uint32_t)(q * mols) << 21 : 0u);
        }
        tp.pat = pat;
    }
#pragma unroll
    for (int k = 0; k < SPT; k++) {
        const int idx = in.ts + k * TBLOCK + tid;
        if (idx < in.te) {
            if (!KEEP_VF) {
                in.v[k] = velm[idx];
                if (pat == 0u) in.meta[k] = a.meta[idx];
                else in.meta[k] = tp.word[k];
            }
            if (LOAD_F) {
                in.fx[k] = a.force[idx];
                in.fy[k] = a.force[idx + a.padded];
                in.fz[k] = a.force[idx + 2 * a.padded];
            }
            if (O::POS) {
                in.p[k] = posq[idx];
                if (PREC == TGNH_PREC_MIXED) in.c[k] = pcorr[idx];       // K :443-445
            }
            if (O::DO_MOVE) in.pd[k] = pdelta[idx];
        } else if (!KEEP_VF) {
            in.v[k] = mk4((mixed)0, (mixed)0, (mixed)0, (mixed)0);       // w = 0: treated as massless, never stored
            in.meta[k] = 0u;
        }
    }
}

// One tile, loaded into `cur`, through the operations OPS (A3/A4, A6, A7, A8, A10).  Ends with the LDS images free.
// reuse_img (step_kernel): the velocity image and the COM table of this very tile are still in LDS from the pass before.
template <int PREC, int OPS, int GB>
__device__ __forceinline__ void tile_body(const TileArgs& a, TileEnv<PREC, GB>& e, const TileIn<PREC>& cur, const int trace_tile,
                                          const bool reuse_img = false) {
    typedef typename Prec<PREC>::real real;
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::real4 real4;
    typedef typename Prec<PREC>::mixed4 mixed4;
    typedef OpsOf<OPS> O;
    typedef TileEnv<PREC, GB> E;
    constexpr bool DO_SCALE = O::DO_SCALE, DO_KICK = O::DO_KICK, DO_DRIFT = O::DO_DRIFT, DO_KE = O::DO_KE, DO_PD = O::DO_PD;
    constexpr bool DO_MOVE = O::DO_MOVE, DO_PREKICK = O::DO_PREKICK, NEED_F = O::NEED_F, POS = O::POS, VEL_W = O::VEL_W;
    (void)trace_tile;
    mixed4* const sv = e.sv; mixed4* const scom = e.scom; mixed4* const sx = e.sx;
    const double* const s_scale = e.s_scale;
    const int tid = e.tid, G = e.G;
    const bool use_com = e.use_com;
    const bool hardwall = POS && (a.hardwall != 0);
    const mixed dt = e.dt, fscale = e.fscale, s_com = e.s_com, s_drude = e.s_drude;
    double (&ke_g)[E::GBR] = e.ke_g;
    double& ke_com = e.ke_com; double& ke_drude = e.ke_drude;
    double* const wbins = e.wbins0 + (tid >> 6) * G;
    mixed4* __restrict__ velm = reinterpret_cast<mixed4*>(a.velm);
    real4* __restrict__ posq = reinterpret_cast<real4*>(a.posq);
    float4* __restrict__ pcorr = reinterpret_cast<float4*>(a.posq_corr);
    mixed4* __restrict__ pdelta = reinterpret_cast<mixed4*>(a.pos_delta);
    auto st_img = [&](mixed4* img, int i, const mixed4& u) { E::st_img(img, i, u); };
    auto ld_img = [&](const mixed4* img, int i) -> mixed4 { return E::ld_img(img, i); };
    (void)G; (void)s_com; (void)s_drude; (void)dt; (void)fscale; (void)wbins; (void)ke_com; (void)ke_drude; (void)ke_g;
    (void)posq; (void)pcorr; (void)pdelta; (void)velm; (void)s_scale;

    const int ts = cur.ts, te = cur.te;
    const int rs = cur.rs, nres = cur.nres;
    TRACE_WAIT(); TRACE(3 + 4 * trace_tile);

    mixed4 v[SPT];
    uint32_t meta[SPT];
    long long fx[SPT], fy[SPT], fz[SPT];
    mixed px[SPT], py[SPT], pz[SPT];
    real pq[SPT];
    mixed4 pd[SPT];
    bool ok[SPT];
#pragma unroll
    for (int k = 0; k < SPT; k++) {
        ok[k] = ts + k * TBLOCK + tid < te;
        v[k] = cur.v[k];
        meta[k] = cur.meta[k];
        if (NEED_F) { fx[k] = cur.fx[k]; fy[k] = cur.fy[k]; fz[k] = cur.fz[k]; }
        if (POS) {
            px[k] = cur.p[k].x; py[k] = cur.p[k].y; pz[k] = cur.p[k].z; pq[k] = cur.p[k].w;
            if (PREC == TGNH_PREC_MIXED) { px[k] += (mixed)cur.c[k].x; py[k] += (mixed)cur.c[k].y; pz[k] += (mixed)cur.c[k].z; }
        }
        if (DO_MOVE) pd[k] = cur.pd[k];
    }
    // One fp64 division per slot: the mass.  The LDS images carry it in .w (0 = massless), so the per-molecule walk
    // and the pair arithmetic multiply by masses instead of dividing by inverse masses again (K forms RECIP(w) in
    // every kernel; an fp64 reciprocal is ~15 VALU instructions and these launches are VALU-heavy at small sizes).
    mixed mass[SPT];
#pragma unroll
    for (int k = 0; k < SPT; k++) mass[k] = v[k].w != 0 ? rcp_(v[k].w) : (mixed)0;
    if (DO_PREKICK) {                                            // the pending half kick (A7), as below
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            if (v[k].w != 0) half_kick<ForceCast>(v[k].x, v[k].y, v[k].z, v[k].w, fscale, fx[k], fy[k], fz[k]);
        }
    }
    auto img = [&](int k) { return mk4(v[k].x, v[k].y, v[k].z, mass[k]); };

    bool lds_read = false;   // some lane may still be reading sv/scom of this tile

    // ---------------- A6: rescale (K :249-301 ; Ref :516-541) ----------------
    if (DO_SCALE) {
      if (!reuse_img) {
#pragma unroll
        for (int k = 0; k < SPT; k++) st_img(sv, k * TBLOCK + tid, img(k));
        __syncthreads();
        if (use_com) {
            for (int r = tid; r < nres; r += TBLOCK) {            // K :86-111
                const int2 rt = r == tid ? cur.rt : a.res_table[rs + r];
                if (rt.x < 0) { scom[r] = reinterpret_cast<const mixed4*>(a.big_com)[-rt.x - 1]; continue; }   // molecule longer than a tile
                const int first = rt.y - ts;
                mixed cx = 0, cy = 0, cz = 0, cm = 0;
                for (int j = 0; j < rt.x; j++) {
                    const mixed4 u = ld_img(sv, first + j);
                    const mixed m = u.w;                       // mass (0 for massless sites)
                    cx += u.x * m; cy += u.y * m; cz += u.z * m; cm += m;
                }
                const mixed w = rcp_(cm);
                scom[r] = mk4(cx * w, cy * w, cz * w, w);
            }
            __syncthreads();
        }
      }
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            const uint32_t m = meta[k];
            const uint32_t role = m & 3u, g = (m >> 2) & 255u;
            mixed cx = 0, cy = 0, cz = 0;
            if (use_com) { const mixed4 c = scom[m >> 21]; cx = c.x; cy = c.y; cz = c.z; }
            const mixed s_g = (mixed)s_scale[g];
            if (role == ROLE_NORMAL) {
                if (v[k].w != 0) {                               // K :260-265
                    const mixed rx = v[k].x - cx, ry = v[k].y - cy, rz = v[k].z - cz;
                    v[k].x = s_g * rx + s_com * (v[k].x - rx);
                    v[k].y = s_g * ry + s_com * (v[k].y - ry);
                    v[k].z = s_g * rz + s_com * (v[k].z - rz);
                }
            } else {                                             // K :270-300
                // Written from the lane's own point of view (self s, partner p), which needs no role selects:
                // with cm = (r_s m_s + r_p m_p)/M and K's rel = r_parent - r_drude, both
                //   v_drude'  = s_g cm - s_D rel m_parent/M + s_COM v_com      (K :292-294)
                //   v_parent' = s_g cm + s_D rel m_drude/M  + s_COM v_com      (K :295-297)
                // read  v_s' = s_g cm + s_D (r_s - r_p) m_p/M + s_COM (v_s - r_s).
                const int pl = k * TBLOCK + tid + (int)((m >> 10) & 2047u) - 1024;
                const mixed4 u = ld_img(sv, pl);           // partner velocity, .w = partner mass
                const mixed rsx = v[k].x - cx, rsy = v[k].y - cy, rsz = v[k].z - cz;
                const mixed rpx = u.x - cx, rpy = u.y - cy, rpz = u.z - cz;
                const mixed invTot = rcp_(mass[k] + u.w);
                const mixed msf = invTot * mass[k], mpf = invTot * u.w;
                const mixed sdp = s_drude * mpf;
                v[k].x = s_g * (rsx * msf + rpx * mpf) + sdp * (rsx - rpx) + s_com * (v[k].x - rsx);
                v[k].y = s_g * (rsy * msf + rpy * mpf) + sdp * (rsy - rpy) + s_com * (v[k].y - rsy);
                v[k].z = s_g * (rsz * msf + rpz * mpf) + sdp * (rsz - rpz) + s_com * (v[k].z - rsz);
            }
        }
        lds_read = true;
    }

    TRACE(4 + 4 * trace_tile);
    // ---------------- A8 (constrained path): x += posDelta, v = posDelta/dt (K :435-466) ---
    if (DO_MOVE) {
        const double invStep = 1.0 / a.dt;                       // K :436
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            if (v[k].w != 0) {
                px[k] += pd[k].x; py[k] += pd[k].y; pz[k] += pd[k].z;
                v[k].x = (mixed)(invStep * pd[k].x);
                v[k].y = (mixed)(invStep * pd[k].y);
                v[k].z = (mixed)(invStep * pd[k].z);
            }
        }
    }

    // ---------------- A7: half kick (K :307-365 ; Ref :548-584) ----------------
    // Per-particle form v += (dt/2) F/m.  The reference writes the pair kick in
    // COM/relative coordinates; that is algebraically the same update
    // (tests/test_oracle.py::test_pair_kick_identity), so no partner access is needed here.
    if (DO_KICK) {
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            if (v[k].w != 0) half_kick<ForceCast>(v[k].x, v[k].y, v[k].z, v[k].w, fscale, fx[k], fy[k], fz[k]);
        }
    }

    // ---------------- A8: drift (Ref :253-258 ; K :322-324, :450-452) ----------------
    if (DO_DRIFT) {
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            if (v[k].w != 0) {
                px[k] += dt * v[k].x; py[k] += dt * v[k].y; pz[k] += dt * v[k].z;
            }
        }
    }
    if (DO_PD) {
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            const int idx = ts + k * TBLOCK + tid;
            if (ok[k]) {
                const bool mv = v[k].w != 0;
                pdelta[idx] = mk4(mv ? dt * v[k].x : (mixed)0, mv ? dt * v[k].y : (mixed)0, mv ? dt * v[k].z : (mixed)0, (mixed)0);
            }
        }
    }

    // ---------------- A10: hard wall (K :471-574 ; Ref :298-363) ----------------
    if (POS && hardwall) {
        if (lds_read) __syncthreads();
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            st_img(sv, k * TBLOCK + tid, img(k));
            st_img(sx, k * TBLOCK + tid, mk4(px[k], py[k], pz[k], (mixed)0));
        }
        __syncthreads();
        const mixed maxd = (mixed)a.max_dist, hws = (mixed)a.hw_scale;
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            const uint32_t m = meta[k];
            const uint32_t role = m & 3u;
            if (role != ROLE_NORMAL) {
                const int pl = k * TBLOCK + tid + (int)((m >> 10) & 2047u) - 1024;
                const mixed4 ux = ld_img(sx, pl);
                const mixed sxd = px[k] - ux.x, syd = py[k] - ux.y, szd = pz[k] - ux.z;     // self - partner
                const mixed d2 = sxd * sxd + syd * syd + szd * szd;
                if (d2 > maxd * maxd) {                           // r > max  <=>  rInv*max < 1 (K :490): the rest only for violators
                    const mixed4 uv = ld_img(sv, pl);
                    const bool is_d = role == ROLE_DRUDE;
                    const mixed4 vel1 = is_d ? v[k] : uv, vel2 = is_d ? uv : v[k];
                    const mixed dx = is_d ? sxd : -sxd, dy = is_d ? syd : -syd, dz = is_d ? szd : -szd;   // Drude - parent (K :487)
                    const mixed r = sqrt_(d2);
                    const mixed rInv = rcp_(r);
                    if (rInv * maxd < (mixed)0.5) atomicOr(a.status, 1u);     // Ref :311-312
                    const mixed bx = dx * rInv, by = dy * rInv, bz = dz * rInv;
                    const mixed mass1 = is_d ? mass[k] : uv.w, mass2 = is_d ? uv.w : mass[k];   // image .w = mass
                    const mixed deltaR = r - maxd;
                    mixed deltaT = dt;
                    mixed dotvr1 = vel1.x * bx + vel1.y * by + vel1.z * bz;
                    const mixed vp1x = vel1.x - bx * dotvr1, vp1y = vel1.y - by * dotvr1, vp1z = vel1.z - bz * dotvr1;
                    // K :527-571 (a massless parent, K :504-526, cannot occur: tgnh_create rejects massless pair members)
                    const mixed invTot = rcp_(mass1 + mass2);
                    mixed dotvr2 = vel2.x * bx + vel2.y * by + vel2.z * bz;
                    const mixed vp2x = vel2.x - bx * dotvr2, vp2y = vel2.y - by * dotvr2, vp2z = vel2.z - bz * dotvr2;
                    const mixed vbCMass = (mass1 * dotvr1 + mass2 * dotvr2) * invTot;
                    dotvr1 -= vbCMass;
                    dotvr2 -= vbCMass;
                    if (dotvr1 != dotvr2) deltaT = deltaR / abs_(dotvr1 - dotvr2);
                    if (deltaT > dt) deltaT = dt;
                    const mixed vBond = hws / sqrt_(mass1);
                    dotvr1 = -dotvr1 * vBond * mass2 * invTot / abs_(dotvr1);
                    dotvr2 = -dotvr2 * vBond * mass1 * invTot / abs_(dotvr2);
                    const mixed dr1 = -deltaR * mass2 * invTot + deltaT * dotvr1;
                    const mixed dr2 = deltaR * mass1 * invTot + deltaT * dotvr2;
                    dotvr1 += vbCMass;
                    dotvr2 += vbCMass;
                    if (is_d) {
                        px[k] += bx * dr1; py[k] += by * dr1; pz[k] += bz * dr1;
                        v[k].x = vp1x + bx * dotvr1; v[k].y = vp1y + by * dotvr1; v[k].z = vp1z + bz * dotvr1;
                    } else {
                        px[k] += bx * dr2; py[k] += by * dr2; pz[k] += bz * dr2;
                        v[k].x = vp2x + bx * dotvr2; v[k].y = vp2y + by * dotvr2; v[k].z = vp2z + bz * dotvr2;
                    }
                }
            }
        }
        lds_read = true;
    }

    TRACE(5 + 4 * trace_tile);
    // ---------------- stores ----------------
#pragma unroll
    for (int k = 0; k < SPT; k++) {
        const int idx = ts + k * TBLOCK + tid;
        if (ok[k]) {
            if (VEL_W || (POS && hardwall)) velm[idx] = v[k];
            if (POS) store_position<PREC>(posq, pcorr, idx, px[k], py[k], pz[k], pq[k]);
        }
    }

    // ---------------- A3/A4: kinetic energies (K :82-200 ; Ref :439-460) ----------------
    if (DO_KE) {
        if (lds_read) __syncthreads();
#pragma unroll
        for (int k = 0; k < SPT; k++) st_img(sv, k * TBLOCK + tid, img(k));
        __syncthreads();
        if (use_com) {
            for (int r = tid; r < nres; r += TBLOCK) {            // K :86-111, :152-158
                const int2 rt = r == tid ? cur.rt : a.res_table[rs + r];
                if (rt.x < 0) { scom[r] = reinterpret_cast<const mixed4*>(a.big_com)[-rt.x - 1]; continue; }   // its M v_com^2 comes from big_com_kernel
                const int first = rt.y - ts;
                mixed cx = 0, cy = 0, cz = 0, cm = 0;
                for (int j = 0; j < rt.x; j++) {
                    const mixed4 u = ld_img(sv, first + j);
                    const mixed m = u.w;                       // mass (0 for massless sites)
                    cx += u.x * m; cy += u.y * m; cz += u.z * m; cm += m;
                }
                const mixed w = rcp_(cm);
                cx *= w; cy *= w; cz *= w;
                scom[r] = mk4(cx, cy, cz, w);
                ke_com += ((double)cx * cx + (double)cy * cy + (double)cz * cz) * (double)cm;     // M v_com^2 (K :154)
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            const uint32_t m = meta[k];
            const uint32_t role = m & 3u, g = (m >> 2) & 255u;
            double cx = 0, cy = 0, cz = 0;
            if (use_com) { const mixed4 c = scom[m >> 21]; cx = c.x; cy = c.y; cz = c.z; }
            double val = 0.0;
            if (role == ROLE_NORMAL) {
                if (v[k].w != 0) {                               // K :161-168
                    const double rx = v[k].x - cx, ry = v[k].y - cy, rz = v[k].z - cz;
                    val = (rx * rx + ry * ry + rz * rz) * (double)mass[k];
                }
            } else if (role == ROLE_DRUDE) {                     // K :171-186 (one lane per pair)
                const int pl = k * TBLOCK + tid + (int)((m >> 10) & 2047u) - 1024;
                const mixed4 u = ld_img(sv, pl);
                const double r1x = v[k].x - cx, r1y = v[k].y - cy, r1z = v[k].z - cz;
                const double r2x = u.x - cx, r2y = u.y - cy, r2z = u.z - cz;
                const double mass1 = mass[k], mass2 = u.w;               // image .w = mass
                const double invTot = rcp_(mass1 + mass2);
                const double m1f = invTot * mass1, m2f = invTot * mass2;
                const double cmx = r1x * m1f + r2x * m2f, cmy = r1y * m1f + r2y * m2f, cmz = r1z * m1f + r2z * m2f;
                const double rlx = r2x - r1x, rly = r2y - r1y, rlz = r2z - r1z;
                val = (cmx * cmx + cmy * cmy + cmz * cmz) * (mass1 + mass2);
                ke_drude += (rlx * rlx + rly * rly + rlz * rlz) * (mass1 * mass2 * invTot);   // reduced mass = 1/invReducedMass (K :178, :185)
            }
            if constexpr (GB > 0) {
#pragma unroll
                for (int b = 0; b < GB; b++) ke_g[b] += (g == (uint32_t)b) ? val : 0.0;
            } else {
                // one pass per distinct group present in this wavefront (usually 1-3): butterfly-sum the lanes of
                // that group, lane 0 adds the sum to the wave's LDS bin.  The order depends on the data only.
                const bool has = role == ROLE_DRUDE || (role == ROLE_NORMAL && v[k].w != 0);
                unsigned long long rem = __ballot(has);
                while (rem) {
                    const int src = __ffsll((long long)rem) - 1;
                    const uint32_t g0 = __shfl(g, src, 64);
                    const bool mine = has && g == g0;
                    const double sg = wave_sum(mine ? val : 0.0);
                    if ((tid & 63) == 0) wbins[g0] += sg;
                    rem &= ~__ballot(mine);
                }
            }
        }
        lds_read = true;
    }
    if (lds_read) __syncthreads();       // LDS image is reused by the next tile
}

}  // namespace tgnh
#endif
