// tgnh_scale_positions.h -- the launchers of tgnh_scale_positions.hip, for the host code of tgnh_scale_positions (tgnh_positions.cpp).
// A header of its own, not lines of tgnh_internal.h: no header the step kernels' unit reads changes with this feature.
#ifndef TGNH_SCALE_POSITIONS_H_
#define TGNH_SCALE_POSITIONS_H_

#include "tgnh_by_index.h"

namespace tgnh {

constexpr int SP_SPAN_SLOTS = 64;            // a span: whole molecules, consecutive slots, one wavefront
constexpr int SP_WAVES = BLOCK / 64;         // spans (fast path) or molecules (table path) per work-group
// (the table path's per-slot pass: index_grid work-groups, tgnh_by_index.h)
inline int sp_wave_grid(int waves) { return (int)(((long long)waves + SP_WAVES - 1) / SP_WAVES); }

struct ScalePosArgs {
    void* posq;                  // real4 [n]
    void* corr;                  // float4 [n], mixed precision only
    void* snap_posq;             // != nullptr: what was read is stored here too (same types)
    void* snap_corr;
    int n;
    double sm1[3];               // scale - 1.0, formed once on the host
    // fast path: span k holds the slots [span_first[k], span_first[k + 1]), bit l of span_heads[k] set where a molecule starts at lane l
    const int* span_first;       // [num_spans + 1]
    const unsigned long long* span_heads;   // [num_spans]
    int num_spans;
    // table path
    const int* mol_of;           // [n] molecule of a slot
    const int* mem_start;        // [num_molecules + 1] into members
    const int* members;          // [n] slots by molecule, ascending within one
    double* shift;               // [3 num_molecules] d of every molecule
    int num_molecules;
};

// the fast path: one launch, a wavefront per span
hipError_t launch_scale_positions_spans(int precision, const ScalePosArgs& a, hipStream_t s);
// the table path: a wavefront per molecule leaves d[3] in a.shift, then one pass by global slot index applies it
hipError_t launch_scale_positions_table(int precision, const ScalePosArgs& a, hipStream_t s);

}  // namespace tgnh

#endif
