// tgnh_vplanes.hip -- the two layout conversions behind the one-launch step's velocity planes.
//
// velm is OpenMM's mixed4 (vx, vy, vz, 1/m).  wstep_kernel reads it twice and writes it once per step, and a third of those bytes
// is the inverse mass, which never changes.  Between flushes of a TGNH_FLAG_DEFER_SCALE | TGNH_FLAG_RESIDENT_STEP sequence -- when
// velm is stale by contract anyway -- the library keeps the velocities in three planes of its own (x | y | z of Prec::mixed, stride
// padded, as the force buffer is laid out) and the kernel takes 1/m from a per-pattern table (tgnh_wave_device.h).  These kernels
// move the velocities there and back; neither does arithmetic.
//   velm -> planes   by wave tile (a wavefront per tile, a lane per slot), because it also checks what the kernel will rely on:
//                    every slot's w IS its pattern entry, bit for bit.  The host reads the verdict once per bind.
//   planes -> velm   by slot; w is read from velm and stored back as read.
//
// A unit of its own so that the step kernels' unit compiles to what it compiled to before.
#include "tgnh_vplanes.h"
#include "tgnh_device_math.h"

namespace tgnh {

__device__ __forceinline__ bool same_bits(const float a, const float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ bool same_bits(const double a, const double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

template <int PREC>
__global__ __launch_bounds__(BLOCK) void velm_to_planes_kernel(const void* __restrict__ velm_, void* __restrict__ planes_, const int2* __restrict__ wave_tile,
                                                               const int num_wtiles, const void* __restrict__ invm_, const int padded,
                                                               uint32_t* __restrict__ mismatch) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    const int lane = (int)threadIdx.x & 63;
    const int t = (int)blockIdx.x * (BLOCK / 64) + ((int)threadIdx.x >> 6);
    if (t >= num_wtiles) return;
    const int ws = wave_tile[t].x, n = wave_tile[t + 1].x - ws;
    if (lane >= n) return;                                               // (a wave tile holds <= 64 slots: tgnh_topology.cpp)
    const int idx = ws + lane;
    const mixed4 v = reinterpret_cast<const mixed4*>(velm_)[idx];
    mixed* __restrict__ planes = reinterpret_cast<mixed*>(planes_);
    planes[idx] = v.x; planes[idx + padded] = v.y; planes[idx + 2 * padded] = v.z;
    if (mismatch) {
        const uint32_t p = (uint32_t)wave_tile[t].y >> 8;                // period | pattern << 8
        const int period = (int)(p & 255u);
        bool same = false;
        if (period) same = same_bits(reinterpret_cast<const mixed*>(invm_)[(p >> 8) * PATTERN_WORDS + (uint32_t)(lane % period)], v.w);
        if (!same) atomicOr(mismatch, 1u);
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void planes_to_velm_kernel(const void* __restrict__ planes_, void* __restrict__ velm_, const int n, const int padded) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    const mixed* __restrict__ planes = reinterpret_cast<const mixed*>(planes_);
    mixed4* __restrict__ velm = reinterpret_cast<mixed4*>(velm_);
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    mixed4 v = velm[i];
    v.x = planes[i]; v.y = planes[i + padded]; v.z = planes[i + 2ll * padded];
    velm[i] = v;
}

hipError_t launch_velm_to_planes(int precision, const void* velm, void* planes, const int2* wave_tile, int num_wtiles,
                                 const void* wpat_invm, int padded, uint32_t* mismatch, hipStream_t s) {
    if (!velm || !planes || !wave_tile || !wpat_invm || num_wtiles < 1 || padded < 1) return hipErrorInvalidValue;
    const int grid = (num_wtiles + BLOCK / 64 - 1) / (BLOCK / 64);
    TGNH_LAUNCH_PREC(velm_to_planes_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, velm, planes, wave_tile, num_wtiles, wpat_invm, padded, mismatch);
    return hipGetLastError();
}

hipError_t launch_planes_to_velm(int precision, const void* planes, void* velm, int n, int padded, hipStream_t s) {
    if (!velm || !planes || n < 1 || padded < n) return hipErrorInvalidValue;
    const int grid = (n + BLOCK - 1) / BLOCK;
    TGNH_LAUNCH_PREC(planes_to_velm_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, planes, velm, n, padded);
    return hipGetLastError();
}

}  // namespace tgnh
