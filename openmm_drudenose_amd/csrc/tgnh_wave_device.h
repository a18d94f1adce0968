// tgnh_wave_device.h -- device code of the wave tiles (wke_kernel, wstep_kernel: tgnh_wave_kernels.h): a wavefront owns <= 64
// consecutive slots that never cut a molecule or a pair, and a private LDS image.  Included by .hip files only.
#ifndef TGNH_WAVE_DEVICE_H_
#define TGNH_WAVE_DEVICE_H_
#include "tgnh_tile_device.h"

namespace tgnh {

// Wave tiles of identical molecules (PATTERN_WORDS, tgnh_internal.h): a lane's position in the pattern is the same in every such
// tile (they all start on a molecule), so the lane keeps its word in a register and fetches it again only when a tile of another
// pattern comes by -- for a water box once per launch.  pat = period | pattern << 8, 0 = this tile's words are read from wmeta.
struct PatternWord {
    uint32_t pat = 0u, word = 0u;
    // also(at): what else the lane keeps of its place `at` in the pattern tables, fetched when the word is
    template <typename Also>
    __device__ __forceinline__ bool of(const TileArgs& a, const uint32_t p, const int lane, Also&& also) {     // wavefront-uniform
        if ((p & 255u) == 0u) return false;
        if (p != pat) {
            const int period = (int)(p & 255u);
            const int q = (int)(((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)period));     // lane div period (never within rounding of an integer)
            const uint32_t at = (p >> 8) * PATTERN_WORDS + (uint32_t)(lane - q * period);
            word = a.wpattern[at];
            also(at);
            pat = p;
        }
        return true;
    }
    __device__ __forceinline__ bool of(const TileArgs& a, const uint32_t p, const int lane) { return of(a, p, lane, [](uint32_t) {}); }
};

// wke_kernel's register image and load (two images in flight, forces only for a kicking pass: its budget of <= 102 VGPRs).
// wstep_kernel has its own below (WStepIn, WaveStep::load_vf: one image that also carries positions, mass and v_com across the
// meeting).
template <int PREC> struct WaveIn {
    typename Prec<PREC>::mixed4 v;
    uint32_t meta;
    long long fx, fy, fz;
};

template <int PREC, int OPS>
__device__ __forceinline__ void wave_load(const TileArgs& a, const int ws, const int n, const bool patterned, const uint32_t pword, const int lane, WaveIn<PREC>& in) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    const mixed4* __restrict__ velm = reinterpret_cast<const mixed4*>(a.velm);
    const int idx = ws + lane;
    mixed4 v = mk4((mixed)0, (mixed)0, (mixed)0, (mixed)0);      // a padding lane: massless, role normal, a molecule of its own -- contributes nothing
    uint32_t meta = 64u << 10;
    long long fx = 0, fy = 0, fz = 0;
    if (lane < n) {
        v = velm[idx];
        if (!patterned) meta = a.wmeta[idx];
        if (OPS & OP_KICK) {
            fx = a.force[idx];
            fy = a.force[idx + a.padded];
            fz = a.force[idx + 2 * a.padded];
        }
    }
    if (patterned && lane < n) meta = pword;
    in.v = v; in.meta = meta; in.fx = fx; in.fy = fy; in.fz = fz;
}

template <int PREC> struct WStepIn {
    typename Prec<PREC>::mixed4 v;
    uint32_t meta;
    long long fx, fy, fz;
    typename Prec<PREC>::real4 p;
    float4 c;
    // formed by the first half of the work on a tile (prepare): mass, centre-of-mass velocity of the slot's molecule
    typename Prec<PREC>::mixed mass, cx, cy, cz;
};

// ---------------------------------------------------------------------------
// The per-tile work of the one-launch step over WAVE tiles (wstep_kernel): a wavefront owns <= 64 consecutive
// slots and a private LDS image (velocity x, y, z, mass; position x, y, z for the hard wall); nothing here waits for another
// wavefront.  load_vf / load_x issue a tile's global loads, prepare forms mass, the half kick (KICK), the image and the
// molecule's centre-of-mass velocity and -- ke -- adds the tile's kinetic energies to the bins (pass 1); finish is pass 2:
// rescale, half kick, drift, hard wall, stores.  The arithmetic per slot is tile_body's / wke_kernel's, expression for expression.
// Reference: K :82-113, :138-200 (COM, bins), :249-301 (rescale), :307-365 (kick), :435-466 (drift), :471-574 (hard wall).
// ---------------------------------------------------------------------------
struct WaveBounds { int ws, y, n, base; };  // first slot; the tile's largest molecule | pattern word << 8; slots; PLANES: the tile's first word of a plane

// PLANES: the velocities are read from and stored to the library's x | y | z planes (TileArgs::vplanes) and a slot's 1/m comes with
// its pattern word.  The planes hold the MASSIVE slots only, packed in slot order, a tile's segment on a 128-byte line: a lane
// with 1/m != 0 finds its word at the tile's base (a scalar load beside the tile's bounds) + its offset (fetched with 1/m, kept
// in one register); a massless lane touches no plane and its image is (0, 0, 0, w = 0) -- what its velocity contributes to every
// sum, v * 0, as long as velm's words were finite (checked on entry, tgnh_vplanes.hip).  Forces, positions and the LDS image keep
// lane = slot offset.  A template parameter, so that the velm form is compiled without a trace of the other (as a launch-uniform
// branch in one kernel the planes' code cost the velm path 2.2 % of its steps/s).
template <int PREC, int GB, bool PLANES = false> struct WaveStep {
    typedef typename Prec<PREC>::real real;
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::real4 real4;
    typedef typename Prec<PREC>::mixed4 mixed4;
    const TileArgs& a;
    TileEnv<PREC, GB>* e;                   // the kinetic-energy bins, in the shape ke_reduce takes them
    const double* s_scale;
    mixed *ix, *iy, *iz, *im, *jx, *jy, *jz;
    mixed4* __restrict__ velm; real4* __restrict__ posq; float4* __restrict__ pcorr;
    // PLANES: x | y | z, and the lane's 1/m and offset into its tile's segment beside its pattern word
    mixed* __restrict__ vpl;
    mixed pinvm;
    int poff;
    int lane, G, nw;
    bool use_com, hardwall;
    mixed dt, fscale;
    PatternWord pw;
    // img: this wavefront's [7][WAVE_SLOTS] LDS image
    __device__ __forceinline__ WaveStep(const TileArgs& a_, TileEnv<PREC, GB>* e_, const double* s_scale_, mixed* img, const int lane_)
        : a(a_), e(e_), s_scale(s_scale_), ix(img), iy(img + WAVE_SLOTS), iz(img + 2 * WAVE_SLOTS), im(img + 3 * WAVE_SLOTS),
          jx(img + 4 * WAVE_SLOTS), jy(img + 5 * WAVE_SLOTS), jz(img + 6 * WAVE_SLOTS),
          velm(reinterpret_cast<mixed4*>(a_.velm)), posq(reinterpret_cast<real4*>(a_.posq)), pcorr(reinterpret_cast<float4*>(a_.posq_corr)),
          vpl(reinterpret_cast<mixed*>(a_.vplanes)), pinvm((mixed)0), poff(0), lane(lane_), G(a_.num_groups), nw(a_.num_wtiles), use_com(a_.use_com != 0), hardwall(a_.hardwall != 0),
          dt((mixed)a_.dt), fscale((mixed)(0.5 * a_.dt / 4294967296.0)) {}     // Cu :295
    __device__ __forceinline__ static void wfence() {      // a wavefront's LDS operations are processed in order: only the compiler is held
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ void bounds(const int ww, WaveBounds& b) const {      // (wavefront-uniform: scalar loads)
        const int at = a.reverse ? nw - 1 - ww : ww;
        const int2* t = a.wave_tile + at;
        b.ws = t[0].x; b.y = t[0].y; b.n = t[1].x - b.ws;
        if (PLANES) b.base = (int)a.wtile_base[at];
    }
    __device__ __forceinline__ void load_vf(const WaveBounds& b, WStepIn<PREC>& in) {          // what pass 1 needs
        const int idx = b.ws + lane;
        const bool patterned = pw.of(a, (uint32_t)b.y >> 8, lane, [&](const uint32_t at) {
            if (PLANES) {
                pinvm = reinterpret_cast<const mixed*>(a.wpat_invm)[at];
                poff = (int)a.wpat_off[((uint32_t)b.y >> 16) * PATTERN_WORDS + (uint32_t)lane];      // (by lane, not by place in the period)
            }
        });
        mixed4 v = mk4((mixed)0, (mixed)0, (mixed)0, (mixed)0);
        uint32_t meta = 64u << 10;
        long long fx = 0, fy = 0, fz = 0;
        if (lane < b.n) {
            if (PLANES) {
                if (pinvm != (mixed)0) {
                    const int vi = b.base + poff;
                    v = mk4(vpl[vi], vpl[vi + a.vstride], vpl[vi + 2 * a.vstride], pinvm);           // (w: the bits velm holds, checked on entry)
                }
            } else v = reinterpret_cast<const mixed4*>(a.velm)[idx];
            if (!patterned) meta = a.wmeta[idx];
            fx = a.force[idx]; fy = a.force[idx + a.padded]; fz = a.force[idx + 2 * a.padded];
        }
        if (patterned && lane < b.n) meta = pw.word;
        in.v = v; in.meta = meta; in.fx = fx; in.fy = fy; in.fz = fz;
    }
    __device__ __forceinline__ void load_x(const WaveBounds& b, WStepIn<PREC>& in) const {           // ... and what pass 2 needs on top
        const int idx = b.ws + lane;
        if (lane < b.n) {
            in.p = reinterpret_cast<const real4*>(a.posq)[idx];
            if (PREC == TGNH_PREC_MIXED) in.c = reinterpret_cast<const float4*>(a.posq_corr)[idx];      // K :443-445
        }
    }
    // first half of the work on a tile: mass, the pending half kick, the wavefront's image, the molecule's centre-of-mass
    // velocity; KE: this tile's kinetic energies go into the bins (pass 1)
    template <bool KICK = true>
    __device__ __forceinline__ void prepare(WStepIn<PREC>& t, const WaveBounds& bd, const bool ke) {
        mixed4& v = t.v;
        const uint32_t m = t.meta;
        t.mass = v.w != 0 ? rcp_(v.w) : (mixed)0;
        if (KICK) {                                                      // A7 (Cu :384-388), per particle; w = 0: c = 0, v unchanged
            const mixed c = fscale * v.w;
            v.x += c * force_as(t.fx, (mixed)0);
            v.y += c * force_as(t.fy, (mixed)0);
            v.z += c * force_as(t.fz, (mixed)0);
        }
        ix[lane] = v.x; iy[lane] = v.y; iz[lane] = v.z; im[lane] = t.mass;
        wfence();
        mixed cx = 0, cy = 0, cz = 0;
        if (use_com) {                                                   // K :86-111: every lane sums its own molecule, in slot order
            const int j = (int)((m >> 17) & 63u), n1 = (int)((m >> 23) & 63u);
            const int first = lane - j;
            mixed px = 0, py = 0, pz = 0, pm = 0;
            for (int k = 0; k < (bd.y & 255); k++) {
                if (k <= n1) {
                    const mixed um = im[first + k];
                    px += ix[first + k] * um; py += iy[first + k] * um; pz += iz[first + k] * um; pm += um;
                }
            }
            const mixed wq = rcp_(pm);
            cx = px * wq; cy = py * wq; cz = pz * wq;
            if (ke && j == 0 && lane < bd.n)                             // M v_com^2 (K :154)
                e->ke_com += ((double)cx * cx + (double)cy * cy + (double)cz * cz) * (double)pm;
        }
        t.cx = cx; t.cy = cy; t.cz = cz;
        if (ke) {                                                        // bins, as wke_kernel (K :138-200)
            const uint32_t role = m & 3u, g = (m >> 2) & 255u;
            const double rx = v.x - cx, ry = v.y - cy, rz = v.z - cz;
            double val = v.w != 0 ? (rx * rx + ry * ry + rz * rz) * (double)t.mass : 0.0;
            if (role == ROLE_DRUDE) {
                const int pl = lane + (int)((m >> 10) & 127u) - 64;
                const double dx = ix[pl] - v.x, dy = iy[pl] - v.y, dz = iz[pl] - v.z;
                const double mass1 = t.mass, mass2 = im[pl];
                const double mu = mass1 * mass2 * rcp_(mass1 + mass2);
                const double d = (dx * dx + dy * dy + dz * dz) * mu;
                e->ke_drude += d;
                val -= d;
            }
#pragma unroll
            for (int b = 0; b < GB; b++) e->ke_g[b] += (g == (uint32_t)b) ? val : 0.0;
        }
    }
    // second half (pass 2): rescale, half kick, drift, hard wall, stores.  The image holds the tile's kicked velocities and masses.
    __device__ __forceinline__ void finish(WStepIn<PREC>& t, const WaveBounds& bd) {
        mixed4 v = t.v;
        const uint32_t m = t.meta;
        const uint32_t role = m & 3u, g = (m >> 2) & 255u;
        const int pl = lane + (int)((m >> 10) & 127u) - 64;
        const mixed mass = t.mass, cx = t.cx, cy = t.cy, cz = t.cz;
        const mixed s_com = (mixed)s_scale[G], s_drude = (mixed)s_scale[G + 1], s_g = (mixed)s_scale[g];
        mixed px = t.p.x, py = t.p.y, pz = t.p.z;
        const real pq = t.p.w;
        if (PREC == TGNH_PREC_MIXED) { px += (mixed)t.c.x; py += (mixed)t.c.y; pz += (mixed)t.c.z; }
        // ---- A6: rescale (K :249-301 ; Ref :516-541), tile_body's expressions
        if (role == ROLE_NORMAL) {
            if (v.w != 0) {
                const mixed rx = v.x - cx, ry = v.y - cy, rz = v.z - cz;
                v.x = s_g * rx + s_com * (v.x - rx);
                v.y = s_g * ry + s_com * (v.y - ry);
                v.z = s_g * rz + s_com * (v.z - rz);
            }
        } else {
            const mixed ux = ix[pl], uy = iy[pl], uz = iz[pl], um = im[pl];      // partner velocity and mass
            const mixed rsx = v.x - cx, rsy = v.y - cy, rsz = v.z - cz;
            const mixed rpx = ux - cx, rpy = uy - cy, rpz = uz - cz;
            const mixed invTot = rcp_(mass + um);
            const mixed msf = invTot * mass, mpf = invTot * um;
            const mixed sdp = s_drude * mpf;
            v.x = s_g * (rsx * msf + rpx * mpf) + sdp * (rsx - rpx) + s_com * (v.x - rsx);
            v.y = s_g * (rsy * msf + rpy * mpf) + sdp * (rsy - rpy) + s_com * (v.y - rsy);
            v.z = s_g * (rsz * msf + rpz * mpf) + sdp * (rsz - rpz) + s_com * (v.z - rsz);
        }
        // ---- A7: half kick (K :307-365) and A8: drift (Ref :253-258 ; K :322-324, :450-452)
        if (v.w != 0) {
            const mixed c = fscale * v.w;
            v.x += c * force_as(t.fx, (mixed)0);
            v.y += c * force_as(t.fy, (mixed)0);
            v.z += c * force_as(t.fz, (mixed)0);
            px += dt * v.x; py += dt * v.y; pz += dt * v.z;
        }
        // ---- A10: hard wall (K :471-574 ; Ref :298-363), tile_body's arithmetic from the lane's own point of view
        if (hardwall) {
            wfence();                                                    // every lane has read its partner's old velocity
            ix[lane] = v.x; iy[lane] = v.y; iz[lane] = v.z;
            jx[lane] = px; jy[lane] = py; jz[lane] = pz;
            wfence();
            if (role != ROLE_NORMAL) {
                const mixed maxd = (mixed)a.max_dist, hws = (mixed)a.hw_scale;
                const mixed sxd = px - jx[pl], syd = py - jy[pl], szd = pz - jz[pl];     // self - partner
                const mixed d2 = sxd * sxd + syd * syd + szd * szd;
                if (d2 > maxd * maxd) {
                    const mixed4 uv = mk4(ix[pl], iy[pl], iz[pl], im[pl]);
                    const bool is_d = role == ROLE_DRUDE;
                    const mixed4 vel1 = is_d ? v : uv, vel2 = is_d ? uv : v;
                    const mixed dx = is_d ? sxd : -sxd, dy = is_d ? syd : -syd, dz = is_d ? szd : -szd;   // Drude - parent (K :487)
                    const mixed r = sqrt_(d2);
                    const mixed rInv = rcp_(r);
                    if (rInv * maxd < (mixed)0.5) atomicOr(a.status, 1u);     // Ref :311-312
                    const mixed bx = dx * rInv, by = dy * rInv, bz = dz * rInv;
                    const mixed mass1 = is_d ? mass : uv.w, mass2 = is_d ? uv.w : mass;
                    const mixed deltaR = r - maxd;
                    mixed deltaT = dt;
                    mixed dotvr1 = vel1.x * bx + vel1.y * by + vel1.z * bz;
                    const mixed vp1x = vel1.x - bx * dotvr1, vp1y = vel1.y - by * dotvr1, vp1z = vel1.z - bz * dotvr1;
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
                        px += bx * dr1; py += by * dr1; pz += bz * dr1;
                        v.x = vp1x + bx * dotvr1; v.y = vp1y + by * dotvr1; v.z = vp1z + bz * dotvr1;
                    } else {
                        px += bx * dr2; py += by * dr2; pz += bz * dr2;
                        v.x = vp2x + bx * dotvr2; v.y = vp2y + by * dotvr2; v.z = vp2z + bz * dotvr2;
                    }
                }
            }
        }
        wfence();                                                        // the next tile's image comes after this tile's reads
        if (lane < bd.n) {
            const int idx = bd.ws + lane;
            if (PLANES) {
                if (pinvm != (mixed)0) {
                    const int vi = bd.base + poff;
                    vpl[vi] = v.x; vpl[vi + a.vstride] = v.y; vpl[vi + 2 * a.vstride] = v.z;
                }
            } else velm[idx] = v;
            store_position<PREC>(posq, pcorr, idx, px, py, pz, pq);
        }
    }
};

}  // namespace tgnh
#endif
