// tgnh_nonbonded.h -- the launchers of tgnh_nonbonded.hip, for the host code of tgnh_set_nonbonded_force / tgnh_compute_nonbonded_force /
// tgnh_get_nonbonded_energy (tgnh_nonbonded.cpp).  A header of its own, as tgnh_bonded.h is: no header the step kernels' unit reads
// changes with this feature.
#ifndef TGNH_NONBONDED_H_
#define TGNH_NONBONDED_H_

#include "tgnh_by_index.h"
#include "tgnh_receivers.h"

namespace tgnh {

constexpr double NB_COULOMB = 138.935456;         // K, kJ nm / (mol e^2): the project's constant (oracle/water_ff.c, tgnh_drude_force.hip)
constexpr double NB_PI = 3.14159265358979323846;
constexpr double NB_CELL_MARGIN = 1.001;          // a cell is at least this many cutoffs wide
constexpr int NB_WAVES = BLOCK / 64;              // wavefronts, and chunks, per work-group of the pair launch
constexpr long long NB_MAX_CELLS = 1LL << 24;     // more cells than this: TGNH_ERR_UNSUPPORTED (the scan is one work-group)

// What every launch of one tgnh_compute_nonbonded_force reads.  The per-slot tables are set-time uploads; the per-cell arrays and
// the sorted copies are rebuilt by every call.
struct NonbondedArgs {
    int n;                          // slots
    const double* par;              // [n][3] charge, sigma, epsilon
    const int* excl_start;          // [n + 1] into excl: a slot's excluded partners, ascending (every exception row, evaluated or not)
    const int* excl;                // [2 ne]
    const int2* excl_range;         // [n] (lowest, highest) excluded partner; (1, 0): none
    const void* posq; const void* posq_corr;
    double box[3];                  // the edges L
    int nc[3], ncells;
    double cutoff2, krf, crf;       // rc^2; krf and crf formed on the host
    int* cell_of;                   // [n]
    int* count;                     // [2 ncells]: the cells' members, then the placement cursors; zeroed before the first launch
    int* cell_start;                // [ncells + 1]
    int2* chunks;                   // [chunk_cap] (cell, first sorted index)
    int* n_chunks;                  // [1]
    int chunk_cap;                  // ncells + ceil(n / 64): the pair launch's wavefronts
    int* placed;                    // [n] slots by cell, any order within one
    double* sorted;                 // [6][n] x, y, z, q, sigma, epsilon in (cell, slot) order
    int* sorted_slot;               // [n]
    int2* sorted_range;             // [n]
    long long* force;               // [3 * padded] fixed point x 2^32, planes x | y | z
    int padded;
    double* rows;                   // want_energy: [pair_grid][4] a work-group's {E_C, E_LJ, 0, 0}; nullptr: forces only
    // tgnh_set_nonbonded_ewald (alpha > 0; 0: the reaction field).  The pair launch takes its Ewald instantiation: erfc pairs
    double alpha, tsp;              // tsp = 2 alpha / sqrt(pi), formed on the host
    double bg_num;                  // ((pi K) (Q Q)) / (2 (alpha alpha)), Q the net charge: E_bg = -(bg_num / V)
    double* ew_misc;                // want_energy: [2] {E_bg, (4 (pi K)) / V} of the call's box, written by the pair launch
};

// The evaluated exceptions and their inverse (tgnh_receivers.h): a term is a row, a role 0 for the row's p1, 1 for its p2
struct NbExceptionArgs {
    const int2* atoms;              // [rows] (p1, p2)
    const double* par;              // [rows][3] chargeProd, sigma, epsilon
    ReceiverTable recv;
    const void* posq; const void* posq_corr;
    long long* force; int padded;
    double* rows;                   // want_energy: [index_grid(recv.n)][4] {E_C, E_LJ, 0, 0}
};

inline int nb_chunk_cap(int n, int ncells) { return ncells + (n + 63) / 64; }
inline int nb_pair_grid(int n, int ncells) { return (nb_chunk_cap(n, ncells) + NB_WAVES - 1) / NB_WAVES; }

// the cell build (4 launches behind a memset of `count`) and the pair launch
hipError_t launch_nonbonded_cells(int precision, const NonbondedArgs& a, hipStream_t s, int stage /* 0..3 */);
hipError_t launch_nonbonded_pairs(int precision, const NonbondedArgs& a, hipStream_t s);
hipError_t launch_nonbonded_exceptions(int precision, const NbExceptionArgs& a, hipStream_t s);
// pair rows [0, n_pair) and exception rows [0, n_exc) (n_exc may be 0) -> out[4] = pair E_C, pair E_LJ, exception E_C, exception E_LJ
hipError_t launch_nonbonded_energy_sum(const double* pair_rows, int n_pair, const double* exc_rows, int n_exc, double* out, hipStream_t s);

}  // namespace tgnh

#endif
