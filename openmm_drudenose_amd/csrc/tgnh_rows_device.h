// tgnh_rows_device.h -- what the passes by global slot index that leave a row of sums per work-group share on the device
// (tgnh_cm_motion.hip, tgnh_drude_stats.hip, tgnh_minimize.hip, the energies of tgnh_drude_force.hip, tgnh_bonded.hip, tgnh_nonbonded.hip).  Included by .hip files only, by none of the step kernels' units.
//
// The order of these sums is a contract -- same bits from any handle over the same slots -- written down
// here: the grid is a function of the slot count alone (index_grid); a thread adds its slots in ascending index order (the
// grid-stride loop, literal in every kernel); a wavefront its lanes with wave_sum; a work-group its wavefronts in wavefront order
// through LDS (sum4_put, the caller's barrier, sum4_total); the one work-group behind the pass the rows by chunk (row_chunk), an
// order that depends on their number only.  No floating-point atomic anywhere.
#ifndef TGNH_ROWS_DEVICE_H_
#define TGNH_ROWS_DEVICE_H_
#include "tgnh_device_math.h"
#include "tgnh_by_index.h"

namespace tgnh {
#pragma clang fp contract(off)       // every sum is rounded on its own, as in the units that include this

static_assert(BLOCK % 64 == 0 && BLOCK >= 4, "whole wavefronts; one thread per sum");
struct Sum4Lds { double wsum[BLOCK / 64][4]; };      // first in a unit's LDS struct

// a thread's four sums -> its wavefront's, in l.  Every thread of the work-group calls this, outside any divergent branch (wave_sum
// reads all 64 lanes).  A barrier of the caller's stands between this and sum4_total.
__device__ __forceinline__ void sum4_put(Sum4Lds& l, double s0, double s1, double s2, double s3) {
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    if ((threadIdx.x & 63) == 0) {
        double* w = l.wsum[threadIdx.x >> 6];
        w[0] = s0; w[1] = s1; w[2] = s2; w[3] = s3;
    }
}
__device__ __forceinline__ double sum4_total(const Sum4Lds& l) {       // threads 0..3: the work-group's sum number threadIdx.x
    double s = l.wsum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; w++) s += l.wsum[w][threadIdx.x];      // wavefront order
    return s;
}
// the two with the barrier between them: a work-group's four sums into its row of rows [grid][4].  Every thread calls this, as it
// calls sum4_put
__device__ __forceinline__ void sum4_store(Sum4Lds& l, double* rows, const double s0, const double s1, const double s2, const double s3) {
    sum4_put(l, s0, s1, s2, s3);
    __syncthreads();
    if (threadIdx.x < 4) rows[4 * (size_t)blockIdx.x + threadIdx.x] = sum4_total(l);
}
// One work-group adds rows [0, nrows): thread t the run of consecutive rows [r0, r1) = [t c, (t + 1) c), c = ceil(nrows / BLOCK), in
// row order; the threads' sums then meet as a work-group's do in the pass.
__device__ __forceinline__ void row_chunk(const int nrows, int& r0, int& r1) {
    const int chunk = (nrows + BLOCK - 1) / BLOCK;
    r0 = min((int)threadIdx.x * chunk, nrows);
    r1 = min(r0 + chunk, nrows);
}

}  // namespace tgnh
#endif
