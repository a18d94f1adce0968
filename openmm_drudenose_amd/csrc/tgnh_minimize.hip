// tgnh_minimize.hip -- the kernels behind tgnh_minimize_iterate: one FIRE iteration (Bitzek et al. 2006) on whatever the bound
// force buffer holds, with the accept / reset decision taken on the device.
//
// The contract is the header's (include/drude_tgnh.h): everything in fp64, every operation rounded on its own.  Two passes by
// global slot index, as the centre-of-mass calls are (tgnh_cm_motion.hip): one that only reads -- forces, the minimiser's velocity
// `work`, the mask byte -- and leaves one row of four sums per work-group, one that reads those and the positions and writes
// positions and `work`.  Between them one work-group adds the rows and one thread takes the decision -- in one launch, or, in a
// sharded run, in two with the caller's all-reduce of the four sums between them.  Nothing here knows tiles, pairs or molecules.
//
// Same bits from any handle over the same slots: the sums are added in the fixed order of tgnh_rows_device.h, the rows by
// min_rowsum_kernel, one work-group.  The count of moving slots is a sum of 1.0s (exact below 2^53).
//
// A unit of its own so that the step kernels' units compile to what they compiled to before.
#include "tgnh_molecule_device.h"
#include "tgnh_minimize.h"
#include "tgnh_rows_device.h"

namespace tgnh {

// every product, quotient and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

struct MinLds {
    Sum4Lds sum;
    double total[4];
};

// a thread's four sums -> l.total, the work-group's.  Called as sum4_put is; a barrier has passed when it returns.
__device__ __forceinline__ void min_block_sums(MinLds& l, double s0, double s1, double s2, double s3) {
    sum4_put(l.sum, s0, s1, s2, s3);
    __syncthreads();
    if (threadIdx.x < 4) l.total[threadIdx.x] = sum4_total(l.sum);
    __syncthreads();
}

__device__ __forceinline__ double min_force(const long long f) { return (double)f / 4294967296.0; }

// forces, work, mask -> rows [gridDim.x][4]: read only, 24 B of force, 24 B of work and the mask byte per moving lane and trip
__global__ __launch_bounds__(BLOCK) void min_sums_kernel(const MinArgs a) {
    __shared__ MinLds l;
    double p = 0.0, ff = 0.0, vv = 0.0, moving = 0.0;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        if (a.mask[it]) {
            const double fx = min_force(a.force[it]), fy = min_force(a.force[it + a.padded]), fz = min_force(a.force[it + 2ll * a.padded]);
            const double vx = a.work[it], vy = a.work[it + a.n], vz = a.work[it + 2ll * a.n];
            p = p + ((fx * vx + fy * vy) + fz * vz);
            ff = ff + ((fx * fx + fy * fy) + fz * fz);
            vv = vv + ((vx * vx + vy * vy) + vz * vz);
            moving = moving + 1.0;
        }
    }
    min_block_sums(l, p, ff, vv, moving);
    if (threadIdx.x < 4) a.rows[4ll * blockIdx.x + threadIdx.x] = l.total[threadIdx.x];
}

// The decision, by one thread: sums = {P, FF, VV, moving} of the whole system.  Once converged != 0 the block stays as it is.
__device__ __forceinline__ void min_decide(const double* __restrict__ sums, MinState* __restrict__ st) {
    if (st->converged != 0) return;
    const double P = sums[0], FF = sums[1], VV = sums[2], M = sums[3];
    const double rms = sqrt(FF / (3.0 * M));
    st->sums[0] = P; st->sums[1] = FF; st->sums[2] = VV; st->sums[3] = M;
    st->rms = rms;
    if (!(__builtin_isfinite(P) && __builtin_isfinite(FF) && __builtin_isfinite(VV) && __builtin_isfinite(M))) { st->converged = -1; return; }
    if (rms <= st->tolerance) { st->converged = 1; return; }
    double aa, bb, dt = st->dt, alpha = st->alpha;
    if (st->iterations == 0) { aa = 1.0; bb = 0.0; }
    else if (P > 0.0) {
        const long long since = st->since_uphill + 1;
        st->since_uphill = since;
        aa = 1.0 - alpha;
        bb = (alpha * sqrt(VV)) / sqrt(FF);                                    // (FF > 0: rms > tolerance >= 0)
        if (since > st->n_min) {
            const double grown = dt * st->f_inc;
            dt = grown < st->dt_max ? grown : st->dt_max;
            alpha = alpha * st->f_alpha;
        }
    } else {
        st->uphill = st->uphill + 1;
        st->since_uphill = 0;
        aa = 0.0; bb = 0.0;
        dt = dt * st->f_dec;
        alpha = st->alpha_start;
    }
    st->iterations = st->iterations + 1;
    st->dt = dt; st->alpha = alpha; st->a = aa; st->b = bb;
}

// rows [0, nrows) -> rows[nrows], the four sums.  One work-group, a thread its chunk of the rows (row_chunk).  decide != 0: thread 0
// goes on to the decision (no all-reduce stands between the two).
__global__ __launch_bounds__(BLOCK) void min_rowsum_kernel(const MinArgs a, const int nrows, const int decide) {
    __shared__ MinLds l;
    int r0, r1;
    row_chunk(nrows, r0, r1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = r0; r < r1; r++) {
        const double* w = a.rows + 4ll * r;
        s0 = s0 + w[0]; s1 = s1 + w[1]; s2 = s2 + w[2]; s3 = s3 + w[3];
    }
    min_block_sums(l, s0, s1, s2, s3);
    if (threadIdx.x < 4) a.rows[4ll * nrows + threadIdx.x] = l.total[threadIdx.x];
    if (decide && threadIdx.x == 0) min_decide(l.total, a.state);
}

__global__ __launch_bounds__(64) void min_decide_kernel(const MinArgs a, const int nrows) {
    if (blockIdx.x == 0 && threadIdx.x == 0) min_decide(a.rows + 4ll * nrows, a.state);
}

// v' = a v + b f;  v'' = v' + dt f;  d = dt v'', capped at max_step;  x' = x + d.  A slot that does not move is neither loaded nor
// written; once the decision has set `converged`, nothing is.
template <int PREC>
__global__ __launch_bounds__(BLOCK) void min_update_kernel(const MinArgs a) {
    const MinState* __restrict__ st = a.state;
    if (st->converged != 0) return;
    const double aa = st->a, bb = st->b, dt = st->dt, max_step = st->max_step;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        if (!a.mask[it]) continue;
        const int i = (int)it;
        const double fx = min_force(a.force[it]), fy = min_force(a.force[it + a.padded]), fz = min_force(a.force[it + 2ll * a.padded]);
        double vx = a.work[it], vy = a.work[it + a.n], vz = a.work[it + 2ll * a.n];
        vx = aa * vx + bb * fx; vy = aa * vy + bb * fy; vz = aa * vz + bb * fz;
        vx = vx + dt * fx; vy = vy + dt * fy; vz = vz + dt * fz;
        double dx = dt * vx, dy = dt * vy, dz = dt * vz;
        const double r = sqrt((dx * dx + dy * dy) + dz * dz);
        if (r > max_step) {
            const double s = max_step / r;
            dx = dx * s; dy = dy * s; dz = dz * s;
        }
        Site<PREC> site;
        site_load<PREC>(a.posq, a.corr, i, site);
        site_store<PREC>(a.posq, a.corr, nullptr, nullptr, i, site, dx, dy, dz);
        a.work[it] = vx; a.work[it + a.n] = vy; a.work[it + 2ll * a.n] = vz;
    }
}

static bool min_args_ok(const MinArgs& a, const int grid) {
    return a.n >= 1 && a.padded >= a.n && grid >= 1 && grid <= INDEX_GRID_CAP && a.force && a.work && a.mask && a.rows && a.state;
}

hipError_t launch_min_sums(const MinArgs& a, int grid, int decide, hipStream_t s) {
    if (!min_args_ok(a, grid)) return hipErrorInvalidValue;
    TGNH_LAUNCH(min_sums_kernel, dim3(grid), dim3(BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(min_rowsum_kernel, dim3(1), dim3(BLOCK), 0, s, a, grid, decide);
    return hipGetLastError();
}

hipError_t launch_min_decide(const MinArgs& a, int grid, hipStream_t s) {
    if (!min_args_ok(a, grid)) return hipErrorInvalidValue;
    TGNH_LAUNCH(min_decide_kernel, dim3(1), dim3(64), 0, s, a, grid);
    return hipGetLastError();
}

hipError_t launch_min_update(int precision, const MinArgs& a, int grid, hipStream_t s) {
    if (!min_args_ok(a, grid) || !a.posq || (precision == TGNH_PREC_MIXED && !a.corr)) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(min_update_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace tgnh
