// tgnh_rescale.hip -- the two small kernels behind tgnh_scale_velocities and tgnh_rescale_to_temperature: one that lays a handful
// of doubles handed over with the launch into device memory, one that turns the summed kinetic energies into rescale factors.
//
// Neither touches a velocity.  The rescale itself (A6: a slot's velocity relative to its molecule's centre of mass by its group's
// factor, the centres of mass by theirs, a pair's relative Drude motion by the Drude factor) is the step's own rescale launch --
// tile_kernel<OP_SCALE> or the gather path's update kernel, through run_tile -- reading its factors from this unit's scratch
// instead of the thermostat block.  The per-slot formula is written once, there.
//
// The contract is the header's (include/drude_tgnh.h).  Per thermostat k, in fp64, every operation rounded on its own:
//   target_k < 0 (RESCALE_INERT: no degrees of freedom)   1
//   KE_k is NaN                                           1, and status bit 4 (what a chain handed a NaN sum sets)
//   KE_k > 0                                              sqrt(target_k / KE_k): one IEEE division, one square root
//   KE_k == 0                                             1
// Thermostats number up to 2048 on the gather path: one work-group walks them, 256 at a time.
//
// A unit of its own so that the step kernels' units compile to what they compiled to before.
#include "tgnh_rescale.h"

namespace tgnh {

// no fused multiply-add (there is no product-and-sum here today; the unit is compiled as the statistics unit is all the same: a
// test restates the rule in numpy)
#pragma clang fp contract(off)

static_assert(RESCALE_PUT_CHUNK == BLOCK, "one thread per value of a chunk");
static_assert(sizeof(RescaleChunk) <= 2048, "a launch carries 4 KiB of arguments at the most");

__global__ __launch_bounds__(BLOCK) void rescale_put_kernel(double* __restrict__ dst, const RescaleChunk c, const int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

__global__ __launch_bounds__(BLOCK) void rescale_factors_kernel(const double* __restrict__ ke, const double* __restrict__ target, const int NT,
                                                                double* __restrict__ factors, uint32_t* __restrict__ status) {
    for (int k = threadIdx.x; k < NT; k += BLOCK) {
        const double t = target[k], e = ke[k];
        double f = 1.0;
        if (!(t < 0.0)) {
            if (e != e) { if (status) atomicOr(status, 16u); }
            else if (e > 0.0) f = sqrt(t / e);
        }
        factors[k] = f;
    }
}

hipError_t launch_rescale_put(double* dst, const double* src, int count, hipStream_t s) {
    if (!dst || !src || count < 1) return hipErrorInvalidValue;
    for (int off = 0; off < count; off += RESCALE_PUT_CHUNK) {
        const int n = count - off < RESCALE_PUT_CHUNK ? count - off : RESCALE_PUT_CHUNK;
        RescaleChunk c{};
        for (int i = 0; i < n; i++) c.v[i] = src[off + i];
        TGNH_LAUNCH(rescale_put_kernel, 1, BLOCK, 0, s, dst + off, c, n);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_rescale_factors(const double* ke, const double* target, int NT, double* factors, uint32_t* status, hipStream_t s) {
    if (!ke || !target || !factors || NT < 1) return hipErrorInvalidValue;
    TGNH_LAUNCH(rescale_factors_kernel, 1, BLOCK, 0, s, ke, target, NT, factors, status);
    return hipGetLastError();
}

}  // namespace tgnh
