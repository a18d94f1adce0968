// tgnh_drude_force.h -- the launchers of tgnh_drude_force.hip, for the host code of tgnh_set_drude_force / tgnh_compute_drude_force /
// tgnh_get_drude_energy (tgnh_drude_force.cpp).  A header of its own, as tgnh_virtual_sites.h is: no header the step kernels' unit
// reads changes with this feature.
#ifndef TGNH_DRUDE_FORCE_H_
#define TGNH_DRUDE_FORCE_H_

#include "tgnh_by_index.h"
#include "tgnh_receivers.h"

namespace tgnh {

// roles of a receiving slot in a term (DrudeForceArgs::recv)
enum : int { DF_P = 0, DF_P1 = 1, DF_P2 = 2, DF_P3 = 3, DF_P4 = 4 };          // in a row: p, p1, p2, p3, p4
enum : int { DF_DRUDE_I = 0, DF_PARENT_I = 1, DF_DRUDE_J = 2, DF_PARENT_J = 3 };   // in a screened pair of rows (i, j)

// The table in the kernel's form, rows in the caller's order (row k is the descriptor's pair k), and its inverse
// (tgnh_receivers.h).  A term below n_rows is that row (its isotropic and anisotropic springs); term n_rows + m is screened pair m.
struct DrudeForceArgs {
    const int4* atoms;              // [n_rows] (p, p1, p2, p3); -1: none
    const int* p4;                  // [n_rows]; -1 where p3 is (the host checked: both or neither)
    const double* k;                // [3][n_rows] planes k1, k2, k3 (k1, k2: the host's zero where the row has no such axis)
    const int2* pair_rows;          // [n_screened] (i, j)
    const double2* pair_par;        // [n_screened] (a = thole / (alpha_i alpha_j)^(1/6), K = C q_i q_j)
    int n_rows, n_screened;
    ReceiverTable recv;             // roles: DF_*
    const void* posq; const void* posq_corr;
    long long* force;               // [3 * padded] fixed point x 2^32, planes x | y | z
    int padded;
    double* rows;                   // want_energy: [grid][4] a work-group's {springs, screened pairs, 0, 0}; nullptr: forces only
};

inline int df_grid(int n_recv) { return index_grid(n_recv); }      // the passes' one grid rule: part of the order the energy is added in

hipError_t launch_drude_force(int precision, const DrudeForceArgs& a, hipStream_t s);
// rows [0, nrows) -> out[4], one work-group
hipError_t launch_drude_energy_sum(const double* rows, int nrows, double* out, hipStream_t s);

}  // namespace tgnh

#endif
