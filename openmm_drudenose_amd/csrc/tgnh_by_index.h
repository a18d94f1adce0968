// tgnh_by_index.h -- the passes by global slot index: their one grid rule, and the rows and launchers of tgnh_velinit.hip,
// tgnh_drude_stats.hip and tgnh_cm_motion.hip for their host code.  No header the step kernels' unit reads changes with these.
#ifndef TGNH_BY_INDEX_H_
#define TGNH_BY_INDEX_H_
#include "tgnh_internal.h"

namespace tgnh {
// work-groups of such a pass, a function of the slot count alone: beyond 1024 x BLOCK = 262 144 slots the threads take the
// grid-stride loop again.  Where a work-group leaves a row of sums, part of the order they are added in (tgnh_rows_device.h)
constexpr int INDEX_GRID_CAP = 1024;
inline int index_grid(int n) { const long long g = ((long long)n + BLOCK - 1) / BLOCK; return (int)(g < INDEX_GRID_CAP ? g : INDEX_GRID_CAP); }

// the velocity draw (tgnh_velinit.hip): velm [n] mixed4, partner [n] as GatherArgs::partner, kT / kTD = kB T / kB T_D
hipError_t launch_velinit(int precision, void* velm, const int* partner, int n, double kT, double kTD,
                          unsigned long long seed, long long first_particle, hipStream_t s);
// Drude pair statistics (tgnh_drude_stats.hip): a read-only pass over posq (+ posq_corr) and the partner table, one row per
// work-group, then one work-group that adds the rows into rows[grid]
struct DrudeStatsRow {
    double sum_d2, dipole[3];
    unsigned long long max_key;              // bit pattern of the largest d2 (orders as the double does: d2 >= 0)
    long long over, pairs;
    int worst, pad;                          // slot of the Drude particle of that pair; 0x7fffffff: the row saw no pair
    long long hist[TGNH_DRUDE_HIST_BINS + 1];
};
hipError_t launch_drude_stats(int precision, const void* posq, const void* posq_corr, const int* partner, int n, double threshold,
                              double hist_max, DrudeStatsRow* rows /*[grid + 1]: the work-groups' rows, then the result*/, int grid, hipStream_t s);
// Centre-of-mass motion (tgnh_cm_motion.hip): a read-only pass over velm, one row per work-group, then one work-group that adds the
// rows into rows[grid]; and the pass that subtracts P / M -- read from `sums` = {M, Px, Py, Pz} on the device, where an all-reduce
// may have added the other ranks' in between -- or the explicit dv[3] (host; sums == nullptr) from every massive slot
struct CmRow {
    double mass, p[3];                       // (the four doubles an all-reduce sums in place: contiguous, first)
    long long massive;                       // slots with w != 0
};
hipError_t launch_cm_momentum(int precision, const void* velm, int n, CmRow* rows /*[grid + 1]: the work-groups' rows, then the result*/, int grid, hipStream_t s);
hipError_t launch_cm_shift(int precision, void* velm, int n, const double* sums, const double* dv, int grid, hipStream_t s);

}  // namespace tgnh
#endif
