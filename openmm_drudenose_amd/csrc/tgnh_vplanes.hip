// tgnh_vplanes.hip -- the two layout conversions behind the one-launch step's velocity planes.
//
// velm is OpenMM's mixed4 (vx, vy, vz, 1/m).  wstep_kernel reads it twice and writes it once per step; a third of those bytes is
// the inverse mass, which never changes, and a massless slot's three words -- one slot in five of an SWM4 water box -- are
// velocities the integrator never uses.  Between flushes of a TGNH_FLAG_DEFER_SCALE | TGNH_FLAG_RESIDENT_STEP sequence -- when
// velm is stale by contract anyway -- the library keeps the velocities of the MASSIVE slots in three planes of its own (x | y | z
// of Prec::mixed, packed in slot order wave tile by wave tile, a tile's segment on a 128-byte line: tgnh_topology.cpp) and the
// kernel takes 1/m and the lane's place in its tile's segment from per-pattern tables (tgnh_wave_device.h).  These kernels move
// the velocities there and back, both by wave tile (a wavefront per tile, a lane per slot); neither does arithmetic.
//   velm -> planes   massive lanes only.  It also checks what the kernel will rely on: every slot's w IS its pattern entry, bit
//                    for bit, and a massless slot's x, y, z are finite (the kernel's image of such a slot is (0, 0, 0, 0), and
//                    v * 0 is the 0 that velm's words give only where v is finite).  The host reads the verdict once per bind.
//   planes -> velm   massive slots only; w is read from velm and stored back as read.  A massless slot of velm is not touched:
//                    what it held on entry it holds after a stay.
//
// A unit of its own so that the step kernels' unit compiles to what it compiled to before.
#include "tgnh_vplanes.h"
#include "tgnh_device_math.h"

namespace tgnh {

__device__ __forceinline__ bool same_bits(const float a, const float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ bool same_bits(const double a, const double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
// (x - x is 0 for a finite x and NaN for a NaN or an infinity)
template <typename T> __device__ __forceinline__ bool finite3(const T x, const T y, const T z) { return x - x == (T)0 && y - y == (T)0 && z - z == (T)0; }

// what the two kernels share: this wavefront's tile, this lane's slot, 1/m and word of a plane (wavefront-uniform up to `lane`)
template <typename mixed> struct PlaneSlot {
    int idx, word;          // slot; its word of plane x (massive lanes)
    mixed invm;             // the table's 1/m (0: massless); meaningful where `patterned`
    bool inside, patterned;
    __device__ __forceinline__ PlaneSlot(const int2* __restrict__ wave_tile, const int num_wtiles, const void* __restrict__ invm_,
                                         const uint32_t* __restrict__ base, const uint32_t* __restrict__ off) {
        const int lane = (int)threadIdx.x & 63;
        const int t = (int)blockIdx.x * (BLOCK / 64) + ((int)threadIdx.x >> 6);
        inside = false; patterned = false; idx = 0; word = 0; invm = (mixed)0;
        if (t >= num_wtiles) return;
        const int ws = wave_tile[t].x, n = wave_tile[t + 1].x - ws;
        if (lane >= n) return;                                           // (a wave tile holds <= 64 slots: tgnh_topology.cpp)
        inside = true;
        idx = ws + lane;
        const uint32_t p = (uint32_t)wave_tile[t].y >> 8;                // period | pattern << 8
        const int period = (int)(p & 255u);
        if (!period) return;
        patterned = true;
        invm = reinterpret_cast<const mixed*>(invm_)[(p >> 8) * PATTERN_WORDS + (uint32_t)(lane % period)];
        word = (int)(base[t] + off[(p >> 8) * PATTERN_WORDS + (uint32_t)lane]);
    }
};

template <int PREC>
__global__ __launch_bounds__(BLOCK) void velm_to_planes_kernel(const void* __restrict__ velm_, void* __restrict__ planes_, const int2* __restrict__ wave_tile,
                                                               const int num_wtiles, const void* __restrict__ invm_, const uint32_t* __restrict__ base,
                                                               const uint32_t* __restrict__ off, const int stride, uint32_t* __restrict__ mismatch) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    const PlaneSlot<mixed> s(wave_tile, num_wtiles, invm_, base, off);
    if (!s.inside) return;
    const mixed4 v = reinterpret_cast<const mixed4*>(velm_)[s.idx];
    mixed* __restrict__ planes = reinterpret_cast<mixed*>(planes_);
    if (s.patterned && s.invm != (mixed)0) { planes[s.word] = v.x; planes[s.word + stride] = v.y; planes[s.word + 2 * stride] = v.z; }
    if (mismatch) {
        bool same = s.patterned && same_bits(s.invm, v.w);
        if (same && s.invm == (mixed)0) same = finite3(v.x, v.y, v.z);
        if (!same) atomicOr(mismatch, 1u);
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void planes_to_velm_kernel(const void* __restrict__ planes_, void* __restrict__ velm_, const int2* __restrict__ wave_tile,
                                                               const int num_wtiles, const void* __restrict__ invm_, const uint32_t* __restrict__ base,
                                                               const uint32_t* __restrict__ off, const int stride) {
    typedef typename Prec<PREC>::mixed mixed;
    typedef typename Prec<PREC>::mixed4 mixed4;
    const PlaneSlot<mixed> s(wave_tile, num_wtiles, invm_, base, off);
    if (!s.inside || !s.patterned || s.invm == (mixed)0) return;
    const mixed* __restrict__ planes = reinterpret_cast<const mixed*>(planes_);
    mixed4* __restrict__ velm = reinterpret_cast<mixed4*>(velm_);
    mixed4 v = velm[s.idx];
    v.x = planes[s.word]; v.y = planes[s.word + stride]; v.z = planes[s.word + 2 * stride];
    velm[s.idx] = v;
}

static bool planes_args_ok(const void* velm, const void* planes, const int2* wave_tile, int num_wtiles, const void* wpat_invm,
                           const uint32_t* wtile_base, const uint32_t* wpat_off, int stride) {
    return velm && planes && wave_tile && wpat_invm && wtile_base && wpat_off && num_wtiles >= 1 && stride >= 1;
}

hipError_t launch_velm_to_planes(int precision, const void* velm, void* planes, const int2* wave_tile, int num_wtiles,
                                 const void* wpat_invm, const uint32_t* wtile_base, const uint32_t* wpat_off, int stride,
                                 uint32_t* mismatch, hipStream_t s) {
    if (!planes_args_ok(velm, planes, wave_tile, num_wtiles, wpat_invm, wtile_base, wpat_off, stride)) return hipErrorInvalidValue;
    const int grid = (num_wtiles + BLOCK / 64 - 1) / (BLOCK / 64);
    TGNH_LAUNCH_PREC(velm_to_planes_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, velm, planes, wave_tile, num_wtiles, wpat_invm, wtile_base, wpat_off, stride, mismatch);
    return hipGetLastError();
}

hipError_t launch_planes_to_velm(int precision, const void* planes, void* velm, const int2* wave_tile, int num_wtiles,
                                 const void* wpat_invm, const uint32_t* wtile_base, const uint32_t* wpat_off, int stride, hipStream_t s) {
    if (!planes_args_ok(velm, planes, wave_tile, num_wtiles, wpat_invm, wtile_base, wpat_off, stride)) return hipErrorInvalidValue;
    const int grid = (num_wtiles + BLOCK / 64 - 1) / (BLOCK / 64);
    TGNH_LAUNCH_PREC(planes_to_velm_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, planes, velm, wave_tile, num_wtiles, wpat_invm, wtile_base, wpat_off, stride);
    return hipGetLastError();
}

}  // namespace tgnh
