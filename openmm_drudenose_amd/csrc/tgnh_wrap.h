// tgnh_wrap.h -- the launchers of tgnh_wrap.hip, for the host code of tgnh_wrap_molecules and tgnh_write_frame (tgnh_frames.cpp).
// A header of its own, not lines of tgnh_internal.h: no header the step kernels' unit reads changes with this feature.
#ifndef TGNH_WRAP_H_
#define TGNH_WRAP_H_

#include "tgnh_scale_positions.h"

namespace tgnh {

struct WrapArgs {
    void* posq;                  // real4 [n]; read only by the frame launches
    void* corr;                  // float4 [n], mixed precision only
    int n;
    double box[6];               // ax, bx, by, cx, cy, cz of the reduced form: by value, a recorded launch keeps the box it was recorded with
    // span form: the molecule table's spans (ScalePosArgs), and for a frame without Drude slots two more words per span
    const int* span_first;       // [num_spans + 1]
    const unsigned long long* span_heads;   // [num_spans]
    int num_spans;
    const int* span_out;         // [num_spans] output index of the span's first kept slot
    const unsigned long long* span_drude;   // [num_spans] bit l: lane l of the span is a Drude slot
    // table form
    const int* mol_of;           // [n]
    const int* mem_start;        // [num_molecules + 1]
    const int* members;          // [n]
    double* shift;               // [3 num_molecules] d of every molecule (+0.0 three times: not moved)
    int num_molecules;
    // the frame
    const int* out_index;        // [n] table form and plain frame without Drude slots: j of a slot, -1 for a Drude slot; nullptr: j = i
    float* out;                  // component k of output index j at out[k * plane + j * step]
    long long plane, step;       // planar: (stride, 1); interleaved: (1, 3)
    long long count;             // output indices: every j written is below it
    double unit;
    int skip_drude;              // span form: span_out / span_drude give j
};

// in place: every molecule whose centre lies outside the cell moved by whole box vectors; nothing else is written
hipError_t launch_wrap_spans(int precision, const WrapArgs& a, hipStream_t s);
hipError_t launch_wrap_table(int precision, const WrapArgs& a, hipStream_t s);
// read only: the coordinates the wrap would leave, times unit, as floats into a.out
hipError_t launch_frame_spans(int precision, const WrapArgs& a, hipStream_t s);
hipError_t launch_frame_table(int precision, const WrapArgs& a, hipStream_t s);
// ... and without a wrap: by slot index, no molecules
hipError_t launch_frame_plain(int precision, const WrapArgs& a, hipStream_t s);

}  // namespace tgnh

#endif
