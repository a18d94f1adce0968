// tgnh_chain_kernels.h -- the one-work-group kernels of the DrudeTGNHIntegrator step: the Nose-Hoover chains with the fixed-order sum
// of the work-groups' partial rows in front of them (chain_kernel, rowsum_kernel, chain_long_kernel, chain_dualnh_long_kernel;
// the chain numerics: tgnh_chain_device.h), and the small kernels beside the streaming passes: the centre of mass of molecules
// longer than a tile (big_com_kernel), the plain kinetic-energy query.  Part of the translation unit tgnh_kernels.hip:
// holds kernels and non-inline host functions, to be included there and nowhere else.
//
// Reference semantics followed (scychon/openmm_drudeNose):
//   K  = platforms/cuda/src/kernels/drudeTGNH.cu
//   Cu = platforms/cuda/src/CudaDrudeTGNHKernels.cpp
//   Ref= platforms/reference/src/ReferenceDrudeTGNHKernels.cpp
#ifndef TGNH_CHAIN_KERNELS_H_
#define TGNH_CHAIN_KERNELS_H_
#include "tgnh_chain_device.h"
#include "tgnh_slot_device.h"

namespace tgnh {

// ---------------------------------------------------------------------------
// chain_kernel: cross-work-group KE sum (fixed order) + Nose-Hoover chain (A5)
// One work-group.  TGNH: lane itg owns thermostat itg (Cu :558-650).
// dualNH: lane 0 runs the reference's coupled, interleaved arrays (Ref :467-504),
// including its indexing quirk when useDrudeNHChains is false.
// The chain variables are copied into registers (numNHChains <= 4, fully unrolled) or
// LDS (longer chains) for the S-fold loop and written back once: with them left in
// global memory every `etaDot[i] *= expfac` was a dependent HBM round trip.
// ---------------------------------------------------------------------------
constexpr int CHAIN_LDS_DOUBLES = 2048;

// The part of chain_kernel before the chain itself: commit of a staged block, fixed-order sum of the partial rows, the
// exchange's send / wait.  Shared with rowsum_kernel below.
__device__ __forceinline__ void chain_prologue(const ChainArgs& a, double (*sred)[MAX_GROUPS + 2], double* s_chain, double* s_ke) {
    const ChainLayout& L = a.L;
    const int NT = L.NT, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* st = a.st;
    if (a.commit) {                  // take over the block an in-kernel chain staged (everything but the KE sums)
        for (int i = tid; i < L.total; i += BLOCK)
            if (i < L.off_ke_red || i >= L.off_ke_red + NT) st[i] = a.stage[i];
        __syncthreads();
    }
    if (a.do_sum) {
        // Fixed-order sum of the work-group partials: lane `tid` owns partials tid, tid+256, ...; every load of a
        // lane is issued before the first add (one memory latency, not one per partial), then a 64-lane sum
        // and a 4-wave LDS hop.  The order never depends on timing, so the sums are reproducible bit for bit.
        constexpr int PER = GRID_CAP / BLOCK;
        double acc[MAX_GROUPS + 2];
#pragma unroll
        for (int b = 0; b < MAX_GROUPS + 2; b++) acc[b] = 0.0;
        if (NT <= 4) {
            double val[PER][4];
#pragma unroll
            for (int j = 0; j < PER; j++) {
                const int p = tid + j * BLOCK;
#pragma unroll
                for (int b = 0; b < 4; b++) val[j][b] = (p < a.nparts && b < NT) ? a.partials[(size_t)p * NT + b] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < PER; j++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[b] += val[j][b];
        } else {
#pragma unroll
            for (int b = 0; b < MAX_GROUPS + 2; b++) {
                if (b < NT) {
                    double val[PER];
#pragma unroll
                    for (int j = 0; j < PER; j++) { const int p = tid + j * BLOCK; val[j] = p < a.nparts ? a.partials[(size_t)p * NT + b] : 0.0; }
#pragma unroll
                    for (int j = 0; j < PER; j++) acc[b] += val[j];
                }
            }
        }
        for (int p = tid; p < a.nbig; p += BLOCK) {                  // rows of the molecules longer than a tile
#pragma unroll
            for (int b = 0; b < MAX_GROUPS + 2; b++)
                if (b < NT) acc[b] += a.partials[((size_t)GRID_CAP + p) * NT + b];
        }
#pragma unroll
        for (int b = 0; b < MAX_GROUPS + 2; b++) {
            if (b < NT) {
                const double s = wave_sum(acc[b]);
                if (lane == 0) sred[wv][b] = s;
            }
        }
        __syncthreads();
        if (tid < NT) {
            double s = 0.0;
            for (int w = 0; w < BLOCK / 64; w++) s += sred[w][tid];
            st[L.off_ke_red + tid] = s;
            s_ke[tid] = s;
        }
        __syncthreads();
    } else if (tid < NT) {
        s_ke[tid] = st[chain_ke_src(a) + tid];   // summed (and all-reduced) by an earlier launch, or carried over from the last chain
    }
    // A tail sum that gave up on a row leaves NaN (wke_kernel) and sets status bit 4 on ITS rank; behind an all-reduce every rank
    // holds that NaN now, and says so itself -- no rank integrates on silently with a clean status word
    // (not for sums carried over from the last chain, ke_carry: a system without any Drude pair carries the reference's own 0/0
    // in its Drude thermostat, harmless there -- Cu :597-605 with drudeDof = 0)
    if (tid < NT && a.status && !a.ke_carry && s_ke[tid] != s_ke[tid]) atomicOr(a.status, 16u);
    if (a.x_send) xchg_send(a.x, NT, tid, BLOCK, s_chain, tid < NT ? s_ke[tid] : 0.0);
    if (a.x_wait) {
        __syncthreads();
        if (tid < 64) {
            const double tot = xchg_wait_sum(a.x, NT, tid, s_chain);
            if (tid < NT) { s_ke[tid] = tot; st[L.off_ke_red + tid] = tot; }
        }
        __syncthreads();
    }
}

// The row sum alone (do_chain == 0: the chain itself runs inside the next rescale launch): its own small kernel.  A launch
// starts with a cold instruction cache, and behind a pass that has streamed a gigabyte through the L2 and the Infinity Cache
// its code comes from HBM: what a one-work-group launch costs is mostly the cache lines of code on its path.  Inside
// chain_kernel (27 000 lines of ISA with every chain length inlined) that path jumped across the whole kernel.
__global__ __launch_bounds__(BLOCK) void rowsum_kernel(const ChainArgs a) {
    __shared__ double sred[BLOCK / 64][MAX_GROUPS + 2];
    __shared__ double s_chain[2 * XCHG_MAX_WORLD * XCHG_NT_PAD > 64 ? 2 * XCHG_MAX_WORLD * XCHG_NT_PAD : 64];
    __shared__ double s_ke[MAX_GROUPS + 2];
    chain_prologue(a, sred, s_chain, s_ke);
}

__global__ __launch_bounds__(BLOCK) void chain_kernel(const ChainArgs a) {
    __shared__ double sred[BLOCK / 64][MAX_GROUPS + 2];
    __shared__ double s_chain[CHAIN_LDS_DOUBLES];
    __shared__ double s_ke[MAX_GROUPS + 2];
    const ChainLayout& L = a.L;
    const int NT = L.NT, tid = threadIdx.x;
    double* st = a.st;
    CHAIN_TRACE(0);
    chain_prologue(a, sred, s_chain, s_ke);
    if (!a.do_chain) return;
    if (!a.do_sum) __syncthreads();
    CHAIN_TRACE(1);
    if (L.mode == TGNH_MODE_TGNH) {
        // real thermostats on lanes 0..NT-2 of wave 0, the Drude thermostat on lane 0 of wave 1: the two code
        // paths then run side by side on two SIMDs instead of one after the other under one exec mask
        int itg = -1;
        if (tid < NT - 1) itg = tid;
        else if (tid == 64) itg = NT - 1;
        if (itg >= 0) {
            switch (L.C) {
                case 1: { Chain1Regs r = chain1_load(a, a.st, itg); r.ke = s_ke[itg]; chain1_run(a, r, a.st, true, nullptr, itg); } break;   // the arithmetic of the in-kernel chain
                case 2: run_tgnh<2>(a, a.st, a.st, true, nullptr, itg, s_chain, s_ke[itg]); break;
                case 3: run_tgnh<3>(a, a.st, a.st, true, nullptr, itg, s_chain, s_ke[itg]); break;
                case 4: run_tgnh<4>(a, a.st, a.st, true, nullptr, itg, s_chain, s_ke[itg]); break;
                default: run_tgnh<0>(a, a.st, a.st, true, nullptr, itg, s_chain, s_ke[itg]); break;   // host checked NT*(4C+1) <= CHAIN_LDS_DOUBLES
            }
        }
        if (tid == 0) {                                              // Cu :493-497
            double s = 0.0;
            for (int i = 0; i < NT; i++) s += s_ke[i];
            st[L.off_kesum] = 0.5 * s;
        }
    } else if (L.C == 1) {
        // one link: with useDrudeNHChains two independent one-link chains, the code of the TGNH ones (Chain1Map);
        // without, the same two lanes coupled by one shuffle per sub-step (chain1q_run)
        if (tid < 3) {
            Chain1Regs r = chain1_load(a, a.st, tid); r.ke = s_ke[tid];
            if (L.c1_quirk) chain1q_run(a, r, a.st, true, nullptr, tid);
            else chain1_run(a, r, a.st, true, nullptr, tid);
        }
        if (tid == 64) st[L.off_kesum] = 0.5 * (s_ke[0] + s_ke[2]);                  // Ref :586-588 (cached KE)
    } else if (tid == 0) {
        switch (L.C) {
            case 1: run_dualnh<1>(a, a.st, a.st, true, nullptr, s_chain, s_ke[0], s_ke[1], s_ke[2]); break;
            case 2: run_dualnh<2>(a, a.st, a.st, true, nullptr, s_chain, s_ke[0], s_ke[1], s_ke[2]); break;
            case 3: run_dualnh<3>(a, a.st, a.st, true, nullptr, s_chain, s_ke[0], s_ke[1], s_ke[2]); break;
            case 4: run_dualnh<4>(a, a.st, a.st, true, nullptr, s_chain, s_ke[0], s_ke[1], s_ke[2]); break;
            default: run_dualnh<0>(a, a.st, a.st, true, nullptr, s_chain, s_ke[0], s_ke[1], s_ke[2]); break;               // host checked 4*(2C+2) <= CHAIN_LDS_DOUBLES
        }
    }
    CHAIN_TRACE(2);
}
// Chains of 5-16 links (TGNH; ten is the reference test's value, TestReferenceDrudeTGNHIntegrator.cpp:166): a kernel per chain
// length with the links of a thermostat in the REGISTERS of its lane, every loop unrolled -- run_tgnh<CC>, the form of the chains
// of 2-4 links (no range test inside the loop, the exponentials that repeat within a sub-step taken once, the wide form when an
// equilibrating box leaves the short polynomial's range).  A thermostat's half step is 2 C S link updates, each waiting for the one
// before (the sweeps of Cu :566-571 / :586-592 bounce from end to end), run by one wavefront that issues one fp64 instruction per
// ~8 cycles: what it costs is instructions per update.  A link per lane (round 3's form, removed: profiles/r04_chain_cost.md) paid per update two
// DPP moves for the neighbour's value, a range-tested exponential in EVERY lane and four conditional moves to commit in one: ~340
// instructions per sub-step of ten links against ~150 here.  Kernels of their own so that chain_kernel's code stays what it was
// (a launch starts with a cold instruction cache); a thermostat per lane, the Drude thermostat on the second wavefront.
template <int CC>
__global__ __launch_bounds__(BLOCK) void chain_long_kernel(const ChainArgs a) {
    __shared__ double sred[BLOCK / 64][MAX_GROUPS + 2];
    __shared__ double s_chain[2 * XCHG_MAX_WORLD * XCHG_NT_PAD > 64 ? 2 * XCHG_MAX_WORLD * XCHG_NT_PAD : 64];
    __shared__ double s_ke[MAX_GROUPS + 2];
    const ChainLayout& L = a.L;
    const int NT = L.NT, tid = threadIdx.x;
    chain_prologue(a, sred, s_chain, s_ke);
    if (!a.do_sum) __syncthreads();
    int itg = -1;
    if (tid < NT - 1) itg = tid;
    else if (tid == 64) itg = NT - 1;
    if (itg >= 0) run_tgnh<CC>(a, a.st, a.st, true, nullptr, itg, nullptr, s_ke[itg]);
    if (tid == 0) {                                                  // Cu :493-497
        double s = 0.0;
        for (int i = 0; i < NT; i++) s += s_ke[i];
        a.st[L.off_kesum] = 0.5 * s;
    }
}
// dualNH, chains of 5-16 links: ten links WITHOUT useDrudeNHChains are the values of the reference's own test
// (TestReferenceDrudeTGNHIntegrator.cpp:166), i.e. the coupled chain of Ref :476-503 with eleven moving entries.  chain_kernel runs
// such chains as the transcription on LDS-resident vectors (run_dualnh<0>: every access a ~100-cycle round trip on a path that is
// serial by nature); here the entries live in one lane's REGISTERS and the exponentials are the fast chains' polynomials
// (dualnh_quirk_fast<CC>), and with useDrudeNHChains the two independent chains take a lane each (run_dualnh_pair<CC>: lanes 0
// and 2 through chain_both_fast).  The transcription stays behind as what runs when an argument leaves the polynomials' range.
template <int CC>
__global__ __launch_bounds__(BLOCK) void chain_dualnh_long_kernel(const ChainArgs a) {
    __shared__ double sred[BLOCK / 64][MAX_GROUPS + 2];
    __shared__ double s_chain[CHAIN_LDS_DOUBLES];
    __shared__ double s_ke[MAX_GROUPS + 2];
    const ChainLayout& L = a.L;
    const int tid = threadIdx.x;
    chain_prologue(a, sred, s_chain, s_ke);
    if (!a.do_sum) __syncthreads();
    if (tid >= 64) return;
    bool done = false;
    if (L.use_drude_chains != 0) {
        bool ok = false;
        if (tid == 0 || tid == 2) ok = run_dualnh_pair<CC>(a, a.st, a.st, true, nullptr, tid, s_ke[0], s_ke[1], s_ke[2]);
        done = __shfl((int)ok, 0, 64) != 0;                          // (the same answer in both lanes: chain_fast votes)
    } else if (tid == 0) {
        done = dualnh_quirk_fast<CC, true>(a, a.st, a.st, true, nullptr, s_ke[0], s_ke[1], s_ke[2]);
    }
    if (!done && tid == 0) run_dualnh<0, true, false>(a, a.st, a.st, true, nullptr, s_chain, s_ke[0], s_ke[1], s_ke[2]);
}

// ---------------------------------------------------------------------------
// big_com_kernel: COM velocity of the molecules longer than a tile (K :82-113 for those), one work-group each.
// kick = 1 gives the COM after the half kick that the KE launch is about to apply: sum m v' = sum (m v + dt/2 F).
// Also leaves the molecule's M v_com^2 (K :152-158) in its own partial row.
// ---------------------------------------------------------------------------
template <int PREC>
__global__ __launch_bounds__(BLOCK) void big_com_kernel(const BigComArgs a) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    __shared__ double sred[BLOCK / 64][4];
    const mixed4* __restrict__ velm = reinterpret_cast<const mixed4*>(a.velm);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const mixed fscale = (mixed)(0.5 * a.dt / 4294967296.0);
    for (int b = blockIdx.x; b < a.n; b += gridDim.x) {
        const int2 rt = a.table[b];
        double sx = 0, sy = 0, sz = 0, sm = 0;
        for (int j = tid; j < rt.x; j += BLOCK) {
            const int i = rt.y + j;
            const mixed4 v = velm[i];
            if (v.w != 0) {
                mixed vx = v.x, vy = v.y, vz = v.z;
                if (a.kick) {
                    const mixed c = fscale * v.w;
                    vx += c * (mixed)a.force[i]; vy += c * (mixed)a.force[i + a.padded]; vz += c * (mixed)a.force[i + 2 * a.padded];
                }
                const mixed m = rcp_(v.w);
                sx += (double)(vx * m); sy += (double)(vy * m); sz += (double)(vz * m); sm += (double)m;
            }
        }
        sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); sm = wave_sum(sm);
        if (lane == 0) { sred[wv][0] = sx; sred[wv][1] = sy; sred[wv][2] = sz; sred[wv][3] = sm; }
        __syncthreads();
        if (tid == 0) {
            double x = 0, y = 0, z = 0, m = 0;
            for (int w = 0; w < BLOCK / 64; w++) { x += sred[w][0]; y += sred[w][1]; z += sred[w][2]; m += sred[w][3]; }
            const double wi = 1.0 / m;
            x *= wi; y *= wi; z *= wi;
            reinterpret_cast<mixed4*>(a.big_com)[b] = mk4((mixed)x, (mixed)y, (mixed)z, (mixed)wi);
            for (int k = 0; k < a.NT; k++) a.partials[(size_t)b * a.NT + k] = 0.0;
            const mixed cx = (mixed)x, cy = (mixed)y, cz = (mixed)z, cw = (mixed)wi;     // as the tiles will read it
            a.partials[(size_t)b * a.NT + a.G] = ((double)cx * cx + (double)cy * cy + (double)cz * cz) / (double)cw;
        }
        __syncthreads();
    }
}

hipError_t launch_big_com(int precision, const BigComArgs& a, hipStream_t s) {
    int grid = a.n < 1 ? 1 : (a.n > 1024 ? 1024 : a.n);
    TGNH_LAUNCH_PREC(big_com_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// plain / time-shifted kinetic energy (A12): 1/2 sum (v + F ts /m)^2 m
// Cu :656 (ts = 0) ; Ref :70-98 (ts = dt/2, no constraints)
// ---------------------------------------------------------------------------
template <int PREC>
__global__ __launch_bounds__(BLOCK) void plain_ke_kernel(const void* velm_, const long long* force, int n, int padded,
                                                         double ts, double* out) {
    typedef typename Prec<PREC>::mixed4 mixed4;
    __shared__ double sred[BLOCK / 64];
    const mixed4* __restrict__ velm = reinterpret_cast<const mixed4*>(velm_);
    const double fs = ts / 4294967296.0;
    double e = 0.0;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const mixed4 v = velm[i];
        if (v.w != 0) {
            double vx = v.x, vy = v.y, vz = v.z;
            if (ts != 0.0) {
                const double c = fs * (double)v.w;
                vx += c * (double)force[i]; vy += c * (double)force[i + padded]; vz += c * (double)force[i + 2 * padded];
            }
            e += (vx * vx + vy * vy + vz * vz) / (double)v.w;
        }
    }
    e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < BLOCK / 64; w++) s += sred[w];
        out[1 + blockIdx.x] = s;                 // one partial per work-group: no atomics, the order of the sum is fixed below
    }
}

// out[0] = 1/2 sum of the nparts work-group partials out[1 ..], in index order: the query is reproducible bit for bit
__global__ __launch_bounds__(BLOCK) void plain_ke_sum_kernel(double* out, int nparts) {
    __shared__ double sred[BLOCK / 64];
    double e = 0.0;
    for (int i = threadIdx.x; i < nparts; i += BLOCK) e += out[1 + i];
    e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < BLOCK / 64; w++) s += sred[w];
        out[0] = 0.5 * s;
    }
}

hipError_t launch_chain(const ChainArgs& a, hipStream_t s) {
    if (!a.do_chain) TGNH_LAUNCH(rowsum_kernel, dim3(1), dim3(BLOCK), 0, s, a);
    else if (a.L.mode == TGNH_MODE_TGNH && a.L.C > 4 && a.L.C <= 16) {
        switch (a.L.C) {
#define TGNH_LONG(c) case c: TGNH_LAUNCH(chain_long_kernel<c>, dim3(1), dim3(BLOCK), 0, s, a); break;
            TGNH_LONG(5) TGNH_LONG(6) TGNH_LONG(7) TGNH_LONG(8) TGNH_LONG(9) TGNH_LONG(10) TGNH_LONG(11) TGNH_LONG(12)
            TGNH_LONG(13) TGNH_LONG(14) TGNH_LONG(15) TGNH_LONG(16)
#undef TGNH_LONG
        }
    }
    else if (a.L.mode == TGNH_MODE_DUALNH && a.L.C > 4 && a.L.C <= 16) {
        switch (a.L.C) {
#define TGNH_DLONG(c) case c: TGNH_LAUNCH(chain_dualnh_long_kernel<c>, dim3(1), dim3(BLOCK), 0, s, a); break;
            TGNH_DLONG(5) TGNH_DLONG(6) TGNH_DLONG(7) TGNH_DLONG(8) TGNH_DLONG(9) TGNH_DLONG(10) TGNH_DLONG(11) TGNH_DLONG(12)
            TGNH_DLONG(13) TGNH_DLONG(14) TGNH_DLONG(15) TGNH_DLONG(16)
#undef TGNH_DLONG
        }
    }
    else TGNH_LAUNCH(chain_kernel, dim3(1), dim3(BLOCK), 0, s, a);
#ifdef TGNH_TUNING
    // timing experiment only (the thermostat advances twice): the same launch again, its code now in the caches
    static const int again = getenv("TGNH_CHAIN_REPEAT") ? atoi(getenv("TGNH_CHAIN_REPEAT")) : 0;
    for (int r = 0; r < again && a.do_chain; r++) { ChainArgs b = a; b.do_sum = 0; b.commit = 0; b.x_send = 0; b.x_wait = 0; TGNH_LAUNCH(chain_kernel, dim3(1), dim3(BLOCK), 0, s, b); }
#endif
    return hipGetLastError();
}

hipError_t launch_plain_ke(int precision, const void* velm, const long long* force, int n, int padded,
                           double time_shift, double* out, hipStream_t s) {
    int grid = (n + BLOCK - 1) / BLOCK;
    if (grid > PLAIN_KE_PARTS) grid = PLAIN_KE_PARTS;
    if (grid < 1) grid = 1;
    TGNH_LAUNCH_PREC(plain_ke_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, velm, force, n, padded, time_shift, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    TGNH_LAUNCH(plain_ke_sum_kernel, dim3(1), dim3(BLOCK), 0, s, out, grid);
    return hipGetLastError();
}

}  // namespace tgnh
#endif
