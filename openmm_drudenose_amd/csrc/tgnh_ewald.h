// tgnh_ewald.h -- the launchers of tgnh_ewald.hip, for the host code of tgnh_set_nonbonded_ewald / tgnh_compute_nonbonded_force /
// tgnh_get_ewald_energy (tgnh_ewald.cpp, tgnh_nonbonded.cpp): the reciprocal sum over an explicit table of vectors and the correction
// for excluded pairs.  The direct-space erfc pairs are tgnh_nonbonded.hip's pair kernels in their Ewald instantiation.  A header
// of its own, as tgnh_nonbonded.h is: no header the step kernels' unit reads changes with this feature.
#ifndef TGNH_EWALD_H_
#define TGNH_EWALD_H_

#include "tgnh_nonbonded.h"

namespace tgnh {

constexpr int EW_PART = 4096;                     // consecutive slots of one part of the structure-factor sum: part of the order of that sum
constexpr int EW_MAX_KMAX = 255;                  // a kmax component above this: TGNH_ERR_ARG
constexpr long long EW_MAX_VECTORS = 1LL << 20;   // more reciprocal vectors than this: TGNH_ERR_UNSUPPORTED
constexpr double EW_PI = NB_PI;

// M = ((2 kx + 1)(2 ky + 1)(2 kz + 1) - 1) / 2: the vectors n != 0, |n_d| <= kmax_d, whose first non-zero component is positive
inline long long ew_num_vectors(const int kmax[3]) { return ((2LL * kmax[0] + 1) * (2LL * kmax[1] + 1) * (2LL * kmax[2] + 1) - 1) / 2; }
inline int ew_parts(int n) { return (n + EW_PART - 1) / EW_PART; }
inline int ew_sum_tiles(int m) { return (m + BLOCK - 1) / BLOCK; }       // work-groups along x of the sum launch: NB_WAVES tiles of 64 vectors each

// What the three launches of the reciprocal part read.  The table of vectors and the rows are set-time allocations; the box is the
// call's.
struct EwaldArgs {
    int n, m, parts;                // slots, reciprocal vectors, ceil(n / EW_PART)
    const int4* kvec;               // [m] (nx, ny, nz, 0), ascending in nx, then ny, then nz
    const double* par;              // [n][3] charge, sigma, epsilon (the nonbonded table's)
    const void* posq; const void* posq_corr;
    double box[3];                  // the edges L
    double a4;                      // 4 (alpha alpha), formed on the host
    double2* part_rows;             // [parts][m] a part's (C, S) of every vector
    double* coef;                   // [m][5] A C, A S, kx, ky, kz: written by the finalise launch, read by the force launch
    double* rows;                   // want_energy: [index_grid(m)][4] a work-group's {sum of A (C C + S S), 0, 0, 0}; nullptr: forces only
    long long* force; int padded;
};

// The exclusion correction in the receiver-table form (tgnh_receivers.h): a term is a row of `atoms`, a role 0 for the row's p1
struct EwaldExclusionArgs {
    const int2* atoms;              // [rows] (p1, p2): every exception row whose particles' charges have a non-zero product
    const double* par;              // [n][3] the nonbonded table's: qq = K (q_p1 q_p2)
    ReceiverTable recv;
    const void* posq; const void* posq_corr;
    double alpha, tsp;              // tsp = 2 alpha / sqrt(pi), formed on the host
    long long* force; int padded;
    double* rows;                   // want_energy: [index_grid(recv.n)][4] {E, 0, 0, 0}
};

hipError_t launch_ewald_exclusions(int precision, const EwaldExclusionArgs& a, hipStream_t s);
hipError_t launch_ewald_reciprocal(int precision, const EwaldArgs& a, hipStream_t s, int stage /* 0 sum, 1 finalise, 2 force */);
// rec rows [0, n_rec) (may be 0) and exclusion rows [0, n_exc) (may be 0) -> out[4] = misc[1] x the rec rows' sum, e_self, misc[0],
// the exclusion rows' sum; misc = {E_bg, 4 pi K / V} as the pair launch of the call left them.  rec_scale != 0 (the mesh sum's rows,
// tgnh_pme.h: one per work-group of its z launch, up to 2^16 / 8 of them): that factor in the place of misc[1]
constexpr int EW_MAX_REC_ROWS = 8192;
hipError_t launch_ewald_energy_sum(const double* rec_rows, int n_rec, double rec_scale, const double* exc_rows, int n_exc, const double* misc, double e_self,
                                   double* out, hipStream_t s);

}  // namespace tgnh

#endif
