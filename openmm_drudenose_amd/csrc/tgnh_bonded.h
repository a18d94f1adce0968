// tgnh_bonded.h -- the launchers of tgnh_bonded.hip, for the host code of tgnh_set_bonded_forces / tgnh_compute_bonded_forces /
// tgnh_get_bonded_energy (tgnh_bonded.cpp).  A header of its own, as tgnh_drude_force.h is: no header the step kernels' unit reads
// changes with this feature.
#ifndef TGNH_BONDED_H_
#define TGNH_BONDED_H_

#include "tgnh_by_index.h"
#include "tgnh_receivers.h"

namespace tgnh {

// role of a receiving slot in a term (BondedArgs::recv): p1, p2, p3, p4 of the term's row
enum : int { BF_P1 = 0, BF_P2 = 1, BF_P3 = 2, BF_P4 = 3 };
constexpr int BONDED_MAX_PERIODICITY = 12;

// The three tables in the kernel's form, rows in the caller's order, and their one inverse (tgnh_receivers.h).  Bonds are numbered
// first, then angles, then torsions: term t < n_bonds is bond t, t < n_bonds + n_angles angle t - n_bonds, else torsion
// t - n_bonds - n_angles.
struct BondedArgs {
    const int2* bond_atoms;         // [n_bonds] (p1, p2)
    const double2* bond_par;        // [n_bonds] (length, k)
    const int4* angle_atoms;        // [n_angles] (p1, p2, p3, 0), p2 the centre
    const double2* angle_par;       // [n_angles] (angle, k)
    const int4* torsion_atoms;      // [n_torsions] (p1, p2, p3, p4)
    const int* torsion_n;           // [n_torsions] periodicity, 1 .. BONDED_MAX_PERIODICITY (the host checked)
    const double* torsion_par;      // [3][n_torsions] planes cos(phase), sin(phase), k: the first two formed on the host at set time
    int n_bonds, n_angles, n_torsions;
    ReceiverTable recv;             // roles: BF_*
    const void* posq; const void* posq_corr;
    long long* force;               // [3 * padded] fixed point x 2^32, planes x | y | z
    int padded;
    double* rows;                   // want_energy: [grid][4] a work-group's {bonds, angles, torsions, 0}; nullptr: forces only
};

inline int bf_grid(int n_recv) { return index_grid(n_recv); }      // the passes' one grid rule: part of the order the energy is added in

hipError_t launch_bonded_forces(int precision, const BondedArgs& a, hipStream_t s);
// rows [0, nrows) -> out[4], one work-group
hipError_t launch_bonded_energy_sum(const double* rows, int nrows, double* out, hipStream_t s);

}  // namespace tgnh

#endif
