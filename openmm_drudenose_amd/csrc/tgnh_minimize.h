// tgnh_minimize.h -- the state block and the launchers of tgnh_minimize.hip, for the host code of tgnh_minimize_* (tgnh_minimize.cpp).
// A header of its own, not lines of tgnh_internal.h: no header the step kernels' unit reads changes with this feature.
#ifndef TGNH_MINIMIZE_H_
#define TGNH_MINIMIZE_H_

#include "tgnh_by_index.h"

namespace tgnh {

// One minimisation's scalars, on the device from tgnh_minimize_begin to tgnh_minimize_end: what the last decision left, the mix
// the update launch behind it reads, and the descriptor's parameters.  Written by one thread (min_decide) and by nobody else.
struct MinState {
    double sums[4];                          // P, FF, VV, moving -- of the last decision
    long long iterations, uphill, since_uphill;
    int converged, n_min;
    double dt, alpha, rms;
    double a, b;                             // v' = a v + b f of the update behind the last decision
    double tolerance, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha;
};

struct MinArgs {
    void* posq;                              // real4 [n]
    void* corr;                              // float4 [n], mixed precision only
    const long long* force;                  // three planes of `padded` words, 2^32 x kJ/mol/nm
    double* work;                            // three planes of n doubles: the minimiser's velocity
    const unsigned char* mask;               // [n] non-zero: the slot moves
    int n, padded;
    double* rows;                            // [grid + 1][4]: a row per work-group of the sums pass, then the four sums (where an all-reduce adds the other ranks')
    MinState* state;
};

// the sums pass and the row sum -> a.rows[grid]; decide != 0: the row sum's launch takes the decision too
hipError_t launch_min_sums(const MinArgs& a, int grid, int decide, hipStream_t s);
// the decision on a.rows[grid] as a launch of its own (behind an all-reduce)
hipError_t launch_min_decide(const MinArgs& a, int grid, hipStream_t s);
hipError_t launch_min_update(int precision, const MinArgs& a, int grid, hipStream_t s);

}  // namespace tgnh

#endif
