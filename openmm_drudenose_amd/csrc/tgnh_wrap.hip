// tgnh_wrap.hip -- the kernels behind tgnh_wrap_molecules and tgnh_write_frame: whole molecules brought back into the periodic cell
// by box vectors, in place or on the way into a compact fp32 frame.
//
// The contract is the header's (include/drude_tgnh.h): per molecule, in fp64 and every operation rounded on its own, S, n and
// c = S / (double)n exactly as tgnh_scale_positions forms them (tgnh_molecule_device.h has the two walks, written once), then
//   kz = floor(c_z / cz);            d = (kz cx, kz cy, kz cz)
//   ky = floor((c_y - d_y) / by);    d_x = d_x + ky bx;   d_y = d_y + ky by
//   kx = floor((c_x - d_x) / ax);    d_x = d_x + kx ax
// A molecule with kx == ky == kz == 0, or with a centroid that is not finite, stays: d = +0.0 and, in place, NOTHING of it is
// written (mixed precision: its hi / lo split is not re-normalised).  Every other molecule: x' = x(i) - d.
//
// Two sinks, one template parameter:
//   in place   x' stored as tgnh_scale_positions stores, both w bit for bit, the store predicated per molecule;
//   frame      (float)((x(i) - d) * unit) at output index j, component k at out[k * plane + j * step]; positions are only read.
// Two forms, as in tgnh_scale_positions.hip and by the same rule (the same bits from either for every molecule of <= 64 members):
//   spans   a wavefront per span of whole molecules; d never leaves the registers.  A frame without Drude slots reads two more
//           words per span -- the output index of its first kept slot and a mask of its Drude lanes -- and j is that index plus a
//           popcount of the kept lanes below: 12 B per span, not 4 B per slot.
//   table   a wavefront per molecule leaves d[3] in the handle's per-molecule scratch; a pass by global slot index follows, which
//           skips the slots whose d is all zero (in place) or writes the frame (j from out_index where Drude slots are left out).
// Without a wrap the frame is one pass by slot index that knows no molecules.
// No floating-point atomic anywhere; nothing here knows tiles, pairs, flags or the step path, and no order of additions depends
// on a grid.  A unit of its own so that the step kernels' units compile to what they compiled to before.
#include "tgnh_molecule_device.h"
#include "tgnh_wrap.h"

namespace tgnh {

// every product, quotient and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

// d of a molecule from its centroid and the box (ax, bx, by, cx, cy, cz); false: it stays, d = +0.0
__device__ __forceinline__ bool wrap_shift(const double (&box)[6], const double cx, const double cy, const double cz, double& dx, double& dy, double& dz) {
    const double kz = floor(cz / box[5]);
    dx = kz * box[3]; dy = kz * box[4]; dz = kz * box[5];
    const double ky = floor((cy - dy) / box[2]);
    dx = dx + ky * box[1]; dy = dy + ky * box[2];
    const double kx = floor((cx - dx) / box[0]);
    dx = dx + kx * box[0];
    const bool moved = isfinite(cx) && isfinite(cy) && isfinite(cz) && (kx != 0.0 || ky != 0.0 || kz != 0.0);
    if (!moved) dx = dy = dz = 0.0;
    return moved;
}

// one coordinate triple into the frame (j < count: the host's tables keep it so; a launch never writes past what was checked)
__device__ __forceinline__ void frame_put(const WrapArgs& a, const long long j, const double x, const double y, const double z) {
    if (j < 0 || j >= a.count) return;
    float* o = a.out + j * a.step;
    o[0] = (float)(x * a.unit);
    o[a.plane] = (float)(y * a.unit);
    o[2 * a.plane] = (float)(z * a.unit);
}

// the span form: a wavefront per span
template <int PREC, bool FRAME>
__device__ __forceinline__ void wrap_span(const WrapArgs& a, SpImage& img) {
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
    double dx, dy, dz;
    const bool moved = wrap_shift(a.box, sx / nn, sy / nn, sz / nn, dx, dy, dz);
    if (FRAME) {
        long long j = first + lane;
        if (a.skip_drude) {
            const unsigned long long drude = a.span_drude[span];
            if ((drude >> lane) & 1ull) return;
            j = (long long)a.span_out[span] + __popcll(~drude & ((1ull << lane) - 1ull));
        }
        frame_put(a, j, s.x - dx, s.y - dy, s.z - dz);
    } else if (moved) {
        site_store<PREC>(a.posq, a.corr, nullptr, nullptr, first + lane, s, -dx, -dy, -dz);      // (x + (-d) is x - d, bit for bit)
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void wr_span_kernel(const WrapArgs a) {
    __shared__ SpImage img;
    wrap_span<PREC, false>(a, img);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void fr_span_kernel(const WrapArgs a) {
    __shared__ SpImage img;
    wrap_span<PREC, true>(a, img);
}

// the table form, first launch: a wavefront per molecule -> shift[3 molecule]
template <int PREC>
__global__ __launch_bounds__(BLOCK) void wr_shift_kernel(const WrapArgs a) {
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
        wrap_shift(a.box, sx / nn, sy / nn, sz / nn, d[0], d[1], d[2]);
    }
}

// the table form, second launch: by global slot index.  A molecule that moves has a component of d that is not zero (kz cz, or
// ky by, or kx ax), one that stays has +0.0 three times: the slots of the second kind are not touched.
template <int PREC, bool FRAME>
__device__ __forceinline__ void wrap_apply(const WrapArgs& a) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const double* d = a.shift + 3 * (long long)a.mol_of[i];      // (inside [0, num_molecules): the table is the host's renumbering)
        const double dx = d[0], dy = d[1], dz = d[2];
        Site<PREC> s;
        if (FRAME) {
            const long long j = a.out_index ? a.out_index[i] : i;
            if (j < 0) continue;
            site_load<PREC>(a.posq, a.corr, i, s);
            frame_put(a, j, s.x - dx, s.y - dy, s.z - dz);
        } else {
            if (dx == 0.0 && dy == 0.0 && dz == 0.0) continue;
            site_load<PREC>(a.posq, a.corr, i, s);
            site_store<PREC>(a.posq, a.corr, nullptr, nullptr, i, s, -dx, -dy, -dz);
        }
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void wr_apply_kernel(const WrapArgs a) { wrap_apply<PREC, false>(a); }

template <int PREC>
__global__ __launch_bounds__(BLOCK) void fr_apply_kernel(const WrapArgs a) { wrap_apply<PREC, true>(a); }

// the frame without a wrap: by global slot index, d = +0.0
template <int PREC>
__global__ __launch_bounds__(BLOCK) void fr_plain_kernel(const WrapArgs a) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const long long j = a.out_index ? a.out_index[i] : i;
        if (j < 0) continue;
        Site<PREC> s;
        site_load<PREC>(a.posq, a.corr, i, s);
        frame_put(a, j, s.x - 0.0, s.y - 0.0, s.z - 0.0);
    }
}

static bool wr_args_ok(int precision, const WrapArgs& a) {
    return a.n >= 1 && a.posq && (precision != TGNH_PREC_MIXED || a.corr);
}
static bool wr_spans_ok(const WrapArgs& a) { return a.num_spans >= 1 && a.num_spans <= a.n && a.span_first && a.span_heads; }
static bool wr_table_ok(const WrapArgs& a) {
    return a.num_molecules >= 1 && a.num_molecules <= a.n && a.mol_of && a.mem_start && a.members && a.shift;
}
// every index frame_put forms lies inside [0, 2 plane + (count - 1) step + 1): the host has checked that many floats behind out
static bool wr_frame_ok(const WrapArgs& a) {
    if (!a.out || a.count < 1 || a.count > a.n || !(a.unit > 0.0)) return false;
    return (a.step == 1 && a.plane >= a.count) || (a.step == 3 && a.plane == 1);
}

hipError_t launch_wrap_spans(int precision, const WrapArgs& a, hipStream_t s) {
    if (!wr_args_ok(precision, a) || !wr_spans_ok(a)) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(wr_span_kernel, precision, dim3(sp_wave_grid(a.num_spans)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wrap_table(int precision, const WrapArgs& a, hipStream_t s) {
    if (!wr_args_ok(precision, a) || !wr_table_ok(a)) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(wr_shift_kernel, precision, dim3(sp_wave_grid(a.num_molecules)), dim3(BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    TGNH_LAUNCH_PREC(wr_apply_kernel, precision, dim3(index_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_frame_spans(int precision, const WrapArgs& a, hipStream_t s) {
    if (!wr_args_ok(precision, a) || !wr_spans_ok(a) || !wr_frame_ok(a) || (a.skip_drude && (!a.span_out || !a.span_drude))) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(fr_span_kernel, precision, dim3(sp_wave_grid(a.num_spans)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_frame_table(int precision, const WrapArgs& a, hipStream_t s) {
    if (!wr_args_ok(precision, a) || !wr_table_ok(a) || !wr_frame_ok(a) || (a.skip_drude && !a.out_index)) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(wr_shift_kernel, precision, dim3(sp_wave_grid(a.num_molecules)), dim3(BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    TGNH_LAUNCH_PREC(fr_apply_kernel, precision, dim3(index_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_frame_plain(int precision, const WrapArgs& a, hipStream_t s) {
    if (!wr_args_ok(precision, a) || !wr_frame_ok(a) || (a.skip_drude && !a.out_index)) return hipErrorInvalidValue;
    TGNH_LAUNCH_PREC(fr_plain_kernel, precision, dim3(index_grid(a.n)), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace tgnh
