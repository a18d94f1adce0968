// tgnh_constraints.h -- the launchers of tgnh_constraints.hip, for the host code of tgnh_apply_constraints / tgnh_apply_velocity_constraints
// (tgnh_constraints.cpp).  A header of its own, not lines of tgnh_internal.h: no header the step kernels' unit reads changes with this feature.
#ifndef TGNH_CONSTRAINTS_H_
#define TGNH_CONSTRAINTS_H_

#include "tgnh_internal.h"

namespace tgnh {

constexpr int CN_MAX_CONSTRAINTS = 3;        // multipliers per cluster: what the direct solve takes (a 3 x 3 system)

// The cluster table, one entry per cluster in each array (lane c reads entry c of every array), rows sorted by the cluster's
// smallest slot index.  A cluster of the canonical form (4 atoms, 6 distances) holds at most three constraints here; the host has
// numbered them 0..K-1 in the canonical pair order and left the rest empty.
struct ConstraintArgs {
    const int4* atoms;        // [n] slot indices, -1 = unused
    const double4* invmass;   // [n] 1 / mass of the four atoms, from the descriptor's masses (0 for an unused atom)
    const double* d2;         // [3][n] planes: squared distance of constraint k (0: no constraint k)
    const uint32_t* pairs;    // [n] bits 4k..4k+1: first atom (0..3) of constraint k, bits 4k+2..4k+3: its second; bits 12..13: K
    int n;                    // (every index of `atoms` is -1 or a slot of the bound arrays: the host checked at set time)
    const void* posq; const void* posq_corr;
    void* velm; void* pos_delta;
    double tol;
    uint32_t* status;         // bit1: a result outside the tolerance
};

inline int cn_grid(int n) { return (int)(((long long)n + BLOCK - 1) / BLOCK); }   // one lane per cluster: no grid-stride loop, no cap

hipError_t launch_constrain_positions(int precision, const ConstraintArgs& a, hipStream_t s);    // on pos_delta
hipError_t launch_constrain_velocities(int precision, const ConstraintArgs& a, hipStream_t s);   // on velm

}  // namespace tgnh

#endif
