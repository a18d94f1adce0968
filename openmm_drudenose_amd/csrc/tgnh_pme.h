// tgnh_pme.h -- the launchers of tgnh_pme.hip, for the host code of tgnh_set_nonbonded_pme / tgnh_compute_nonbonded_force /
// tgnh_get_pme_grids (tgnh_pme.cpp, tgnh_nonbonded.cpp): the reciprocal part of the Ewald sum on a mesh -- B-spline spreading, a 3-D
// FFT of the library's own, the convolution, the force interpolation.  Everything else of the sum (the erfc pairs, the exclusion
// correction, the self and background energies) is tgnh_ewald.h's and tgnh_nonbonded.h's.  A header of its own, as those are: no
// header the step kernels' unit reads changes with this feature.
#ifndef TGNH_PME_H_
#define TGNH_PME_H_

#include "tgnh_ewald.h"

namespace tgnh {

constexpr int PME_ORDER = 5;                      // the B-spline order: a constant, part of the contract
constexpr int PME_MIN_GRID = 6;                   // a grid component below this, or
constexpr int PME_MAX_GRID = 256;                 // above this: TGNH_ERR_ARG.  With PME_FFT_TILE, what bounds a work-group's LDS
constexpr long long PME_MAX_POINTS = 1LL << 24;   // more grid points than this: TGNH_ERR_UNSUPPORTED
constexpr int PME_FFT_TILE = 8;                   // lines a work-group transforms at once: in the y and z passes 8 adjacent x, 128 contiguous bytes a row
constexpr int PME_MAX_STAGES = 8;                 // 256 = 4^4; 162 = 2 3^4 has five; 8 leaves room
constexpr double PME_FIXED = 281474976710656.0;   // 2^48: the charge grid's fixed point; a grid point holds up to 2^15 e of |q w|

// The radices of one axis' transform, in the order the stages run: 4s, then a 2, then 3s, then 5s
struct PmeFftPlan { int n, stages; unsigned char radix[PME_MAX_STAGES]; };
// n = 2^a 3^b 5^c within [PME_MIN_GRID, PME_MAX_GRID] -> true and the plan
inline bool pme_fft_plan(int n, PmeFftPlan* out) {
    PmeFftPlan p{}; p.n = n;
    if (n < PME_MIN_GRID || n > PME_MAX_GRID) return false;
    int m = n;
    const int order[4] = {4, 2, 3, 5};
    for (int r : order)
        while (m % r == 0) {
            if (p.stages == PME_MAX_STAGES) return false;
            p.radix[p.stages++] = (unsigned char)r; m /= r;
        }
    if (m != 1) return false;
    if (out) *out = p;
    return true;
}
// a line in LDS is padded by one element: the y and z passes fill it with a stride of a whole line
inline size_t pme_fft_lds_bytes(int n) { return (size_t)PME_FFT_TILE * ((size_t)n + 1) * sizeof(double2) + (size_t)n * sizeof(double2); }
inline int pme_fft_grid(const int g[3], int pass /* 0 x, 1 y, 2 z */) {
    if (pass == 0) return (g[1] * g[2] + PME_FFT_TILE - 1) / PME_FFT_TILE;
    if (pass == 1) return g[2] * ((g[0] + PME_FFT_TILE - 1) / PME_FFT_TILE);
    return (g[0] * g[1] + PME_FFT_TILE - 1) / PME_FFT_TILE;
}

// What the launches of the mesh part read.  Every buffer is a set-time allocation; the box is the call's.
struct PmeArgs {
    int n;                          // slots
    int grid[3];                    // nx, ny, nz
    PmeFftPlan plan[3];
    const double* par;              // [n][3] charge, sigma, epsilon (the nonbonded table's)
    const void* posq; const void* posq_corr;
    double box[3];                  // the edges L
    double pi2, alpha2;             // pi pi, alpha alpha, formed on the host
    long long* charge;              // [nz][ny][nx] the spread charges x 2^48
    double2* work;                  // [nz][ny][nx] the complex grid the five transform launches work in
    double* potential;              // [nz][ny][nx] phi
    const double2* twiddle[3];      // [N_d] w^k = (cos(2 pi k / N), -sin(2 pi k / N))
    const double* modulus[3];       // [N_d] |b_d(m)|^2 with OpenMM's rule applied
    double* rows;                   // want_energy: [pme_fft_grid(grid, 2)][4] a work-group's {1/2 sum of G |F|^2, 0, 0, 0}; nullptr: forces only
    long long* force; int padded;
};

// stage 0 spread, 1..5 the transform launches (x forward, y forward, z forward x G z inverse, y inverse, x inverse), 6 gather
hipError_t launch_pme(int precision, const PmeArgs& a, hipStream_t s, int stage);

}  // namespace tgnh

#endif
