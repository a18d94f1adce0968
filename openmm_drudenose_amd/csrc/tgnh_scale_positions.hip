// tgnh_scale_positions.hip -- the kernels behind tgnh_scale_positions: every molecule moved rigidly by (scale - 1) x its centroid,
// the coordinate scaling of a Monte Carlo barostat's trial move.
//
// The contract is the header's (include/drude_tgnh.h): per component, in fp64 and every operation rounded on its own,
//   S = the sum of x(i) over the molecule's n members (n <= 64: ascending slot order, left to right from the first member's value),
//   c = S / (double)n,  d = c * (scale - 1.0),  x' = x(i) + d,  stored in the position type (mixed: hi + lo, re-normalised);
// w of posq and of posq_correction is stored back as it was read.  With a snapshot asked for, what was read is stored there as well.
//
// Two paths, the same bits for every molecule of <= 64 members:
//   spans   (sp_span_kernel) every molecule a run of consecutive slots no longer than a wavefront.  The host has cut the slots into
//           spans of whole molecules, <= 64 slots each; a wavefront takes a span, one slot per lane, coalesced.  Each lane leaves its
//           three coordinates in an LDS image private to its wavefront (no work-group barrier: a wavefront runs in lockstep, the fences
//           keep the compiler from moving the reads ahead of the writes, as wke_kernel keeps its look-ups), finds its molecule's first
//           and last lane in the span's 64-bit mask of molecule heads, walks the image from the first member to the last, and stores.
//           One read and one write of the positions; no centroid table in memory.
//   table   everything else (members that are not consecutive, molecules longer than a wavefront).  sp_shift_kernel: a wavefront per
//           molecule gathers the members through the member list -- up to 64 into the LDS image, summed in the order above; beyond,
//           lane l adds members l, l + 64, ... in ascending order and the lanes meet in wave_sum (a fixed order, a function of the
//           member list alone) -- and leaves d[3] in a table.  sp_apply_kernel: by global slot index, x' = x + d[molecule of the slot].
// No floating-point atomic anywhere.  Same bits from any handle over the same slots and the same molecule table: nothing here knows
// tiles, pairs, flags or the step path, and no order of additions depends on a grid.
//
// A unit of its own so that the step kernels' units compile to what they compiled to before.
#include "tgnh_molecule_device.h"

namespace tgnh {

// every product, quotient and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

// (Site, site_load, site_store, the LDS image and the two centroid walks: tgnh_molecule_device.h, shared with tgnh_wrap.hip)

// the fast path: a wavefront per span
template <int PREC>
__global__ __launch_bounds__(BLOCK) void sp_span_kernel(const ScalePosArgs a) {
    __shared__ SpImage img;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long span = (long long)blockIdx.x * SP_WAVES + w;
    if (span >= a.num_spans) return;                             // (a whole wavefront; no work-group barrier below)
    const int first = a.span_first[span], len = a.span_first[span + 1] - first;     // (the host checked: 1 <= len <= 64, the last span ends at n)
    const unsigned long long heads = a.span_heads[span];         // bit 0 is set
    const bool on = lane < len;
    Site<PREC> s;
    s.x = s.y = s.z = 0.0;
    if (on) site_load<PREC>(a.posq, a.corr, first + lane, s);
    double (&im)[3][64] = img.v[w];
    im[0][lane] = s.x; im[1][lane] = s.y; im[2][lane] = s.z;
    wave_image_ready();
    if (!on) return;
    int m0, m1;
    span_molecule(heads, lane, len, m0, m1);
    double sx, sy, sz;
    image_sum(im, m0, m1, sx, sy, sz);
    const double nn = (double)(m1 - m0);
    const double dx = (sx / nn) * a.sm1[0], dy = (sy / nn) * a.sm1[1], dz = (sz / nn) * a.sm1[2];
    site_store<PREC>(a.posq, a.corr, a.snap_posq, a.snap_corr, first + lane, s, dx, dy, dz);
}

// the table path, first launch: a wavefront per molecule -> shift[3 molecule]
template <int PREC>
__global__ __launch_bounds__(BLOCK) void sp_shift_kernel(const ScalePosArgs a) {
    __shared__ SpImage img;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long mol = (long long)blockIdx.x * SP_WAVES + w;
    if (mol >= a.num_molecules) return;                          // (a whole wavefront; no work-group barrier below)
    const int b = a.mem_start[mol], n = a.mem_start[mol + 1] - b;                 // (the host checked: n >= 1, the last molecule ends at a.n)
    double sx, sy, sz;
    members_sum<PREC>(a.posq, a.corr, a.members, b, n, lane, img.v[w], sx, sy, sz);
    if (lane == 0) {
        const double nn = (double)n;
        double* d = a.shift + 3 * mol;
        d[0] = (sx / nn) * a.sm1[0]; d[1] = (sy / nn) * a.sm1[1]; d[2] = (sz / nn) * a.sm1[2];
    }
}

// the table path, second launch: by global slot index
template <int PREC>
__global__ __launch_bounds__(BLOCK) void sp_apply_kernel(const ScalePosArgs a) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const double* d = a.shift + 3 * (long long)a.mol_of[i];      // (inside [0, num_molecules): the table is the host's renumbering)
        Site<PREC> s;
        site_load<PREC>(a.posq, a.corr, i, s);
        site_store<PREC>(a.posq, a.corr, a.snap_posq, a.snap_corr, i, s, d[0], d[1], d[2]);
    }
}

static bool sp_args_ok(int precision, const ScalePosArgs& a) {
    if (a.n < 1 || !a.posq || (precision == TGNH_PREC_MIXED && !a.corr)) return false;
    if (a.snap_posq && precision == TGNH_PREC_MIXED && !a.snap_corr) return false;
    return true;
}

hipError_t launch_scale_positions_spans(int precision, const ScalePosArgs& a, hipStream_t s) {
    if (!sp_args_ok(precision, a) || a.num_spans < 1 || a.num_spans > a.n || !a.span_first || !a.span_heads) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(sp_span_kernel, precision, dim3(sp_wave_grid(a.num_spans)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scale_positions_table(int precision, const ScalePosArgs& a, hipStream_t s) {
    if (!sp_args_ok(precision, a) || a.num_molecules < 1 || a.num_molecules > a.n || !a.mol_of || !a.mem_start || !a.members || !a.shift)
        return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(sp_shift_kernel, precision, dim3(sp_wave_grid(a.num_molecules)), dim3(BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    TGNH_LAUNCH_PREC(sp_apply_kernel, precision, dim3(index_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace tgnh
