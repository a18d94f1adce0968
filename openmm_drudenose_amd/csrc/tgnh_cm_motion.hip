// tgnh_cm_motion.hip -- the three kernels behind tgnh_get_momentum, tgnh_shift_velocities and tgnh_remove_cm_motion: the total mass
// and momentum of the bound velocities summed on the device, and the shift that takes the centre-of-mass velocity off them.
//
// The contract is the header's (include/drude_tgnh.h): per slot with w != 0, m = 1.0 / (double)w and the four terms m, m vx, m vy,
// m vz in fp64, each product rounded on its own; a slot with w == 0 carries no mass, adds nothing and is never written.  Two passes
// by global slot index, as the velocity draw and the Drude statistics are (tgnh_velinit.hip, tgnh_drude_stats.hip): one that only
// reads velm and leaves one row per work-group, one that reads and writes it.  Between them one work-group adds the rows, and -- in a
// sharded run -- the caller's all-reduce adds the ranks' four sums in place.  Nothing here knows tiles, pairs or molecules; the two
// instantiations are the two types velm has: float4 (single precision) and double4 (mixed, double).
//
// Same bits from any handle over the same slots: the sums are added in the fixed order of tgnh_rows_device.h, the rows by
// cm_momentum_sum_kernel, one work-group.  The count of massive slots goes through an integer LDS atomic (a count does not depend
// on the order).  The shift forms v_cm = P / M in every thread from the same two operands: the same bits everywhere, and on every
// rank that was handed the same sums.
//
// A unit of its own so that the step kernels' units compile to what they compiled to before.
#include "tgnh_rows_device.h"

namespace tgnh {

// every product and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

template <typename V4> struct Component;
template <> struct Component<float4> { typedef float type; };
template <> struct Component<double4> { typedef double type; };

struct CmLds {
    Sum4Lds sum;
    unsigned long long massive;
};

// a thread's four sums and its count -> the work-group's row.  Called as sum4_put is, l.massive cleared and a barrier passed before.
__device__ __forceinline__ void cm_block_row(CmLds& l, double s0, double s1, double s2, double s3, const unsigned long long count,
                                             CmRow* __restrict__ row) {
    sum4_put(l.sum, s0, s1, s2, s3);
    if (count) atomicAdd(&l.massive, count);
    __syncthreads();
    if (threadIdx.x < 4) (threadIdx.x == 0 ? row->mass : row->p[threadIdx.x - 1]) = sum4_total(l.sum);
    if (threadIdx.x == 0) row->massive = (long long)l.massive;
}

// velm [n] -> rows [gridDim.x]: read only, 16 B (float4) or 32 B (double4) per lane and trip
template <typename V4>
__global__ __launch_bounds__(BLOCK) void cm_momentum_kernel(const V4* __restrict__ velm, const int n, CmRow* __restrict__ rows) {
    __shared__ CmLds l;
    if (threadIdx.x == 0) l.massive = 0ull;
    __syncthreads();
    double sm = 0.0, px = 0.0, py = 0.0, pz = 0.0;
    unsigned long long massive = 0;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < n; it += (long long)gridDim.x * BLOCK) {
        const V4 v = velm[it];
        if (v.w != 0) {
            const double m = 1.0 / (double)v.w;
            sm = sm + m;
            px = px + m * (double)v.x; py = py + m * (double)v.y; pz = pz + m * (double)v.z;
            massive++;
        }
    }
    cm_block_row(l, sm, px, py, pz, massive, rows + blockIdx.x);
}

// rows [0, nrows) -> *out.  One work-group, a thread its chunk of the rows (row_chunk).
__global__ __launch_bounds__(BLOCK) void cm_momentum_sum_kernel(const CmRow* __restrict__ rows, const int nrows, CmRow* __restrict__ out) {
    __shared__ CmLds l;
    if (threadIdx.x == 0) l.massive = 0ull;
    __syncthreads();
    int r0, r1;
    row_chunk(nrows, r0, r1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    unsigned long long massive = 0;
    for (int r = r0; r < r1; r++) {
        const CmRow& w = rows[r];
        s0 = s0 + w.mass; s1 = s1 + w.p[0]; s2 = s2 + w.p[1]; s3 = s3 + w.p[2];
        massive += (unsigned long long)w.massive;
    }
    cm_block_row(l, s0, s1, s2, s3, massive, out);
}

// v' = (store type)((double)v - d) for every slot with w != 0, rounded once; w is stored back as it was read.  d = P / M from
// sums = {M, Px, Py, Pz} (device), or -- sums == nullptr -- the three values handed over with the launch.  M == 0: nothing is written.
template <typename V4>
__global__ __launch_bounds__(BLOCK) void cm_shift_kernel(V4* __restrict__ velm, const int n, const double* __restrict__ sums,
                                                         double dx, double dy, double dz) {
    typedef typename Component<V4>::type T;
    if (sums) {
        const double M = sums[0];
        if (M == 0.0) return;
        dx = sums[1] / M; dy = sums[2] / M; dz = sums[3] / M;      // (IEEE division of the same operands in every thread)
    }
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < n; it += (long long)gridDim.x * BLOCK) {
        V4 v = velm[it];
        if (v.w != 0) {
            v.x = (T)((double)v.x - dx); v.y = (T)((double)v.y - dy); v.z = (T)((double)v.z - dz);
            velm[it] = v;
        }
    }
}

hipError_t launch_cm_momentum(int precision, const void* velm, int n, CmRow* rows, int grid, hipStream_t s) {
    if (n < 1 || grid < 1 || grid > INDEX_GRID_CAP || !velm || !rows) return hipErrorInvalidValue;
    switch (precision) {
        case TGNH_PREC_SINGLE: TGNH_LAUNCH(cm_momentum_kernel<float4>, grid, BLOCK, 0, s, static_cast<const float4*>(velm), n, rows); break;
        case TGNH_PREC_MIXED:
        case TGNH_PREC_DOUBLE: TGNH_LAUNCH(cm_momentum_kernel<double4>, grid, BLOCK, 0, s, static_cast<const double4*>(velm), n, rows); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cm_momentum_sum_kernel, 1, BLOCK, 0, s, rows, grid, rows + grid);
    return hipGetLastError();
}

hipError_t launch_cm_shift(int precision, void* velm, int n, const double* sums, const double* dv, int grid, hipStream_t s) {
    if (n < 1 || grid < 1 || grid > INDEX_GRID_CAP || !velm || (!sums && !dv)) return hipErrorInvalidValue;
    const double dx = sums ? 0.0 : dv[0], dy = sums ? 0.0 : dv[1], dz = sums ? 0.0 : dv[2];
    switch (precision) {
        case TGNH_PREC_SINGLE: TGNH_LAUNCH(cm_shift_kernel<float4>, grid, BLOCK, 0, s, static_cast<float4*>(velm), n, sums, dx, dy, dz); break;
        case TGNH_PREC_MIXED:
        case TGNH_PREC_DOUBLE: TGNH_LAUNCH(cm_shift_kernel<double4>, grid, BLOCK, 0, s, static_cast<double4*>(velm), n, sums, dx, dy, dz); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace tgnh
