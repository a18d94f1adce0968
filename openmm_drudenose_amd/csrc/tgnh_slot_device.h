// tgnh_slot_device.h -- per-slot formulas and small blocks of the step that several kernels run, each written once: functions that
// know nothing of tiles, LDS or arrays.  The rule a helper lives by: every kernel's ISA stays what it was (tools/kernel_isa.py); the
// register allocator follows statement order, so a helper keeps its callers' order or does not exist.  Included by .hip files only.
//
// Formulas that are still written at each site, with what a helper did to the ISA when it was tried, one at a time:
//   half kick in WaveStep::prepare / ::finish    half_kick below moves registers in 12 of 18 wstep_kernel (neutral in tile_body, wke_kernel)
//   half kick in big_com_kernel, gather_com_kernel   their force loads sit inside the expression; as arguments they are issued earlier
//   half kick in gather_update_kernel             its forces are converted at load time, for both members of a pair: not this shape
//   rescale (lone particle, pair member)          the callers' statements verbatim, by reference: all of tile_kernel's rescale
//                                                 instantiations, step_kernel, wstep_kernel change
//   hard wall (tile_body, WaveStep::finish, gather_update_kernel)   K :527-571 as one function returning dr, v-across, v-along: every caller
//                                                 changes (18 step_kernel, 15 tile_kernel, 18 wstep_kernel, gather), 1/(m1 + m2) passed in or formed in place
//   wave COM walk and bins (wke_kernel, WaveStep::prepare)   wke_kernel (27) and wstep_kernel (18) change: role / group words move
//   tile COM walk (tile_body, twice)              the two walks differ in form (scale in place / in the store): not tried
//   wke_kernel's Bounds / wave_load beside WaveBounds / load_vf   another register image (tgnh_wave_device.h): not tried
#ifndef TGNH_SLOT_DEVICE_H_
#define TGNH_SLOT_DEVICE_H_
#include "tgnh_device_math.h"

namespace tgnh {

// One-time check at tgnh_create that a grid of this size really is resident all at once (the occupancy API can be one work-group
// per compute unit high): every work-group checks in at a counter and waits, bounded, until all have; one that gives up says so.
__device__ __forceinline__ void census(const TileArgs& a) {
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(&a.sync[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned n = 0;
        while (__hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x && ++n < CENSUS_SPIN_LIMIT)
            __builtin_amdgcn_s_sleep(16);
        if (__hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) atomicOr(&a.sync[3], 1u);
    }
}
// Work-group 0 takes over the thermostat block an in-kernel chain of the launch before staged
__device__ __forceinline__ void commit_staged(const TileArgs& a, const int tid, const int nthreads) {
    if (a.commit_len > 0 && blockIdx.x == 0) {
        for (int i = tid; i < a.commit_len; i += nthreads)
            if (i < a.commit_skip || i >= a.commit_skip + a.commit_skip_n) a.commit_dst[i] = a.commit_src[i];
    }
}

// Position store with the mixed-precision split into a float and its correction (K :457-458)
template <int PREC>
__device__ __forceinline__ void store_position(typename Prec<PREC>::real4* posq, float4* pcorr, const int idx, const typename Prec<PREC>::mixed px,
                                               const typename Prec<PREC>::mixed py, const typename Prec<PREC>::mixed pz, const typename Prec<PREC>::real pq) {
    typedef typename Prec<PREC>::real real;
    if (PREC == TGNH_PREC_MIXED) {
        const float hx = (float)px, hy = (float)py, hz = (float)pz;
        posq[idx] = mk4((real)hx, (real)hy, (real)hz, pq);
        pcorr[idx] = make_float4((float)(px - hx), (float)(py - hy), (float)(pz - hz), 0.0f);
    } else {
        posq[idx] = mk4((real)px, (real)py, (real)pz, pq);
    }
}

// A7 (K :307-365 ; Cu :384-388 ; Ref :548-584): half kick of one particle, v += (dt/2) F/m.  fscale = dt/2 / 2^32 (Cu :295), w = 1/m
// (0: v unchanged).  The fixed-point force becomes a floating-point number after the factor is formed -- by a cast (ForceCast: the
// 512-slot tiles) or by force_as (ForceFma: the wave tiles): the same bits, other instructions.
struct ForceCast { template <typename M> __device__ __forceinline__ static M as(const long long f) { return (M)f; } };
struct ForceFma { template <typename M> __device__ __forceinline__ static M as(const long long f) { return force_as(f, (M)0); } };
template <typename CONV, typename M>
__device__ __forceinline__ void half_kick(M& vx, M& vy, M& vz, const M w, const M fscale, const long long fx, const long long fy, const long long fz) {
    const M c = fscale * w;
    vx += c * CONV::template as<M>(fx);
    vy += c * CONV::template as<M>(fy);
    vz += c * CONV::template as<M>(fz);
}

}  // namespace tgnh
#endif
