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
#include "tgnh_device_math.h"
#include "tgnh_scale_positions.h"

namespace tgnh {

// every product, quotient and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

static_assert(BLOCK % 64 == 0 && SP_SPAN_SLOTS == 64, "whole wavefronts; a span is a wavefront's");

// a slot as it lies in memory, and its coordinates as the header defines them
template <int PREC> struct Site {
    typename Prec<PREC>::real4 p;
    float4 c;                                // mixed precision only
    double x, y, z;
};

template <int PREC>
__device__ __forceinline__ void site_load(const ScalePosArgs& a, const int i, Site<PREC>& s) {
    s.p = static_cast<const typename Prec<PREC>::real4*>(a.posq)[i];
    s.x = (double)s.p.x; s.y = (double)s.p.y; s.z = (double)s.p.z;
    if (PREC == TGNH_PREC_MIXED) {
        s.c = static_cast<const float4*>(a.corr)[i];
        s.x = s.x + (double)s.c.x; s.y = s.y + (double)s.c.y; s.z = s.z + (double)s.c.z;
    }
}

// x' = x + d in the position type; the snapshot first, from the registers the slot was read into
template <int PREC>
__device__ __forceinline__ void site_store(const ScalePosArgs& a, const int i, const Site<PREC>& s, const double dx, const double dy, const double dz) {
    typedef typename Prec<PREC>::real4 R4;
    typedef typename Prec<PREC>::real R;
    if (a.snap_posq) {
        static_cast<R4*>(a.snap_posq)[i] = s.p;
        if (PREC == TGNH_PREC_MIXED) static_cast<float4*>(a.snap_corr)[i] = s.c;
    }
    const double nx = s.x + dx, ny = s.y + dy, nz = s.z + dz;
    const R hx = (R)nx, hy = (R)ny, hz = (R)nz;
    static_cast<R4*>(a.posq)[i] = mk4(hx, hy, hz, s.p.w);
    if (PREC == TGNH_PREC_MIXED)
        static_cast<float4*>(a.corr)[i] = make_float4((float)(nx - (double)hx), (float)(ny - (double)hy), (float)(nz - (double)hz), s.c.w);
}

// what a wavefront has written to its LDS image is read by other lanes of the same wavefront
__device__ __forceinline__ void wave_image_ready() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct SpImage { double v[SP_WAVES][3][64]; };       // 6 KiB a work-group: x, y, z of a wavefront's 64 lanes, each wavefront its own

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
    if (on) site_load<PREC>(a, first + lane, s);
    double (&im)[3][64] = img.v[w];
    im[0][lane] = s.x; im[1][lane] = s.y; im[2][lane] = s.z;
    wave_image_ready();
    if (!on) return;
    // this lane's molecule: from the last head at or below the lane to the next head above it (or the span's end)
    const unsigned long long below = heads & ((2ull << lane) - 1ull);            // (lane 63: 2 << 63 wraps to 0, the mask to all ones)
    const int m0 = 63 - __clzll((long long)below);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int m1 = above ? min(lane + __ffsll((long long)above), len) : len;
    double sx = im[0][m0], sy = im[1][m0], sz = im[2][m0];
    for (int k = m0 + 1; k < m1; k++) { sx = sx + im[0][k]; sy = sy + im[1][k]; sz = sz + im[2][k]; }
    const double nn = (double)(m1 - m0);
    const double dx = (sx / nn) * a.sm1[0], dy = (sy / nn) * a.sm1[1], dz = (sz / nn) * a.sm1[2];
    site_store<PREC>(a, first + lane, s, dx, dy, dz);
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
    Site<PREC> s;
    if (n <= 64) {
        s.x = s.y = s.z = 0.0;
        if (lane < n) site_load<PREC>(a, a.members[b + lane], s);
        double (&im)[3][64] = img.v[w];
        im[0][lane] = s.x; im[1][lane] = s.y; im[2][lane] = s.z;
        wave_image_ready();
        sx = im[0][0]; sy = im[1][0]; sz = im[2][0];
        for (int k = 1; k < n; k++) { sx = sx + im[0][k]; sy = sy + im[1][k]; sz = sz + im[2][k]; }     // (every lane: the same additions)
    } else {
        double tx = 0.0, ty = 0.0, tz = 0.0;
        for (int k = lane; k < n; k += 64) {
            site_load<PREC>(a, a.members[b + k], s);
            tx = tx + s.x; ty = ty + s.y; tz = tz + s.z;
        }
        sx = wave_sum(tx); sy = wave_sum(ty); sz = wave_sum(tz);      // (all 64 lanes are here: n is the wavefront's)
    }
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
        site_load<PREC>(a, i, s);
        site_store<PREC>(a, i, s, d[0], d[1], d[2]);
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
    TGNH_LAUNCH_PREC(sp_apply_kernel, precision, dim3(sp_slot_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace tgnh
