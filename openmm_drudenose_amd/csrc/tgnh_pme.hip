// tgnh_pme.hip -- the kernels behind tgnh_set_nonbonded_pme: what tgnh_compute_nonbonded_force adds behind the exclusion correction
// when particle-mesh Ewald is on.  include/drude_tgnh.h (PARTICLE-MESH EWALD) writes the terms one operation a line; this file
// follows it.  Everything in fp64 in every precision, every operation rounded on its own (no fused multiply-add); the only call into
// the device library is the convolution's exp: the B-splines are polynomials and every twiddle factor is an entry of a table
// uploaded at set time.
//
//   pme_spread_kernel   a lane per charged slot (index_grid's grid-stride loop): 125 atomicAdds of 64-bit INTEGERS, llrint((q w) 2^48),
//                       onto the grid the call's memset cleared.  Integer adds commute: the grid's bits depend neither on the order of
//                       arrival nor on the order of the slots (nb_cell_kernel's argument for its counters).  No floating-point atomic.
//   pme_fft_kernel      five launches: x forward (reads the integer grid, x 2^-48), y forward, z forward x G z inverse, y inverse,
//                       x inverse (writes the real phi).  A work-group holds PME_FFT_TILE whole lines in LDS and runs a mixed-radix
//                       (4, 2, 3, 5) Stockham transform on them: per stage a thread reads the R inputs of its butterflies into
//                       registers, a barrier, it writes the R outputs to their autosorted places, a barrier -- one buffer, no
//                       bit reversal.  x lines are contiguous; the y and z passes take 8 adjacent x, so a row of the tile is 128
//                       contiguous bytes, and a line in LDS is padded by one element against the bank conflicts of that fill.
//                       LDS: 8 (N + 1) 16 + 16 N bytes for the axis' twiddles, 37 008 bytes at N = 256 (+ 128 with want_energy).
//   pme_gather_kernel   a lane per charged slot, c outermost, a innermost; each component converted once, then add_to_planes.
// Every sum's order depends on n, the grid and the tables alone.
#include "tgnh_pme.h"
#include "tgnh_receiver_device.h"
#include "tgnh_rows_device.h"

namespace tgnh {

#pragma clang fp contract(off)

namespace {

// One axis of a slot: the first point of its support and the five weights (and derivatives), Essmann's recursion
struct PmeAxis { int i0; double th[PME_ORDER], dth[PME_ORDER]; };

// th of order k - 1 (th[k - 1] == 0) -> order k
template <int K>
__device__ __forceinline__ void pme_raise(double (&th)[PME_ORDER], const double u) {
    const double div = (double)(K - 1);
    th[K - 1] = (u * th[K - 2]) / div;
#pragma unroll
    for (int j = 1; j <= K - 2; j++) th[K - 1 - j] = ((u + (double)j) * th[K - 2 - j] + ((double)(K - j) - u) * th[K - 1 - j]) / div;
    th[0] = ((1.0 - u) * th[0]) / div;
}

__device__ __forceinline__ void pme_axis(const double x, const double L, const int N, PmeAxis& w) {
    const double s = frac_coord(x, L);
    const double t = s * (double)N;
    const double fl = floor(t);
    const double u = t - fl;
    int i0 = (int)fl;
    if (!(i0 >= 0 && i0 <= N)) i0 = 0;                           // (a position that is not finite: the grid index stays inside the grid)
    w.i0 = i0;
    w.th[0] = 1.0 - u; w.th[1] = u; w.th[2] = 0.0; w.th[3] = 0.0; w.th[4] = 0.0;
    pme_raise<3>(w.th, u);
    pme_raise<4>(w.th, u);
    w.dth[0] = -w.th[0];
#pragma unroll
    for (int j = 1; j < PME_ORDER; j++) w.dth[j] = w.th[j - 1] - w.th[j];
    pme_raise<5>(w.th, u);
}

// point j of the axis: (i0 + j) mod N; i0 <= N and j <= 4 < N
__device__ __forceinline__ int pme_point(const int i0, const int j, const int N) {
    const int p = i0 + j;
    return p >= N ? p - N : p;
}

template <bool INV>
__device__ __forceinline__ double2 pme_cmul(const double2 v, double2 w) {
    if (INV) w.y = -w.y;
    return make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
}

// the R-point transform of v in place, natural order; the roots of unity are entries of the axis' table (tw[k N / R])
template <int R, bool INV>
__device__ __forceinline__ void pme_butterfly(double2 (&v)[R], const double2* tw, const int N) {
    if (R == 2) {
        const double2 a = v[0], b = v[1];
        v[0] = make_double2(a.x + b.x, a.y + b.y);
        v[1] = make_double2(a.x - b.x, a.y - b.y);
    } else if (R == 4) {
        const double2 a = make_double2(v[0].x + v[2].x, v[0].y + v[2].y), b = make_double2(v[0].x - v[2].x, v[0].y - v[2].y);
        const double2 c = make_double2(v[1].x + v[3].x, v[1].y + v[3].y), d = make_double2(v[1].x - v[3].x, v[1].y - v[3].y);
        const double2 minus = make_double2(b.x + d.y, b.y - d.x), plus = make_double2(b.x - d.y, b.y + d.x);      // b - i d, b + i d
        v[0] = make_double2(a.x + c.x, a.y + c.y);
        v[1] = INV ? plus : minus;
        v[2] = make_double2(a.x - c.x, a.y - c.y);
        v[3] = INV ? minus : plus;
    } else {
        double2 o[R];
        const int step = N / R;
#pragma unroll
        for (int a = 0; a < R; a++) {
            o[a] = v[0];
#pragma unroll
            for (int b = 1; b < R; b++) {
                const double2 t = a == 0 ? v[b] : pme_cmul<INV>(v[b], tw[((a * b) % R) * step]);
                o[a] = make_double2(o[a].x + t.x, o[a].y + t.y);
            }
        }
#pragma unroll
        for (int a = 0; a < R; a++) v[a] = o[a];
    }
}

// One Stockham stage of radix R on `lines` lines of N elements, `pitch` apart, Ns the product of the radices before it.  Butterfly j
// of a line (j < N / R, k = j mod Ns) reads x[j + b N / R], turns input b by w^(b k N / (Ns R)), transforms, and writes
// y[(j / Ns) Ns R + k + b Ns].  Every thread passes both barriers.
template <int R, bool INV>
__device__ __forceinline__ void pme_fft_stage(double2* buf, const double2* tw, const int lines, const int N, const int pitch, const int Ns) {
    constexpr int ITEMS = (PME_FFT_TILE * PME_MAX_GRID / R + BLOCK - 1) / BLOCK;
    const int per = N / R, total = lines * per, step = N / (Ns * R);
    double2 v[ITEMS][R];
    int out[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int w = (int)threadIdx.x + i * BLOCK;
        out[i] = -1;
        if (w < total) {
            const int t = w / per, j = w - t * per;
            const int hi = j / Ns, k = j - hi * Ns;
            const double2* x = buf + t * pitch + j;
#pragma unroll
            for (int b = 0; b < R; b++) v[i][b] = x[b * per];
#pragma unroll
            for (int b = 1; b < R; b++) v[i][b] = pme_cmul<INV>(v[i][b], tw[(b * k) * step]);
            pme_butterfly<R, INV>(v[i], tw, N);
            out[i] = t * pitch + (hi * Ns) * R + k;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; i++)
        if (out[i] >= 0) {
#pragma unroll
            for (int b = 0; b < R; b++) buf[out[i] + b * Ns] = v[i][b];
        }
    __syncthreads();
}

template <bool INV>
__device__ __forceinline__ void pme_fft_lines(double2* buf, const double2* tw, const int lines, const PmeFftPlan& p, const int pitch) {
    int Ns = 1;
    for (int s = 0; s < p.stages; s++) {
        const int R = p.radix[s];
        if (R == 4) pme_fft_stage<4, INV>(buf, tw, lines, p.n, pitch, Ns);
        else if (R == 2) pme_fft_stage<2, INV>(buf, tw, lines, p.n, pitch, Ns);
        else if (R == 3) pme_fft_stage<3, INV>(buf, tw, lines, p.n, pitch, Ns);
        else pme_fft_stage<5, INV>(buf, tw, lines, p.n, pitch, Ns);
        Ns *= R;
    }
}

// n_d of grid index m, folded into (-N / 2, N / 2]
__device__ __forceinline__ double pme_fold(const int m, const int N) { return (double)(m <= N / 2 ? m : m - N); }

}  // namespace

template <int PREC>
__global__ __launch_bounds__(BLOCK) void pme_spread_kernel(const PmeArgs a) {
    const int nx = a.grid[0], ny = a.grid[1], nz = a.grid[2];
    unsigned long long* __restrict__ grid = reinterpret_cast<unsigned long long*>(a.charge);
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const double q = a.par[3 * (size_t)i];
        if (q == 0.0) continue;
        const Vec3 x = slot_position<PREC>(a.posq, a.posq_corr, i);
        PmeAxis wx, wy, wz;
        pme_axis(x.x, a.box[0], nx, wx);
        pme_axis(x.y, a.box[1], ny, wy);
        pme_axis(x.z, a.box[2], nz, wz);
#pragma unroll
        for (int c = 0; c < PME_ORDER; c++) {
            const size_t pz = (size_t)pme_point(wz.i0, c, nz) * ny;
#pragma unroll
            for (int b = 0; b < PME_ORDER; b++) {
                const size_t row = (pz + pme_point(wy.i0, b, ny)) * nx;
#pragma unroll
                for (int e = 0; e < PME_ORDER; e++) {
                    const double w = (wx.th[e] * wy.th[b]) * wz.th[c];
                    const long long v = llrint((q * w) * PME_FIXED);
                    atomicAdd(grid + row + pme_point(wx.i0, e, nx), (unsigned long long)v);
                }
            }
        }
    }
}

// MODE 0 x forward from the integer grid, 1 y forward, 2 z forward x G z inverse, 3 y inverse, 4 x inverse to phi
template <int MODE, bool ENERGY>
__global__ __launch_bounds__(BLOCK) void pme_fft_kernel(const PmeArgs a) {
    extern __shared__ double2 pme_lds[];
    __shared__ Sum4Lds sums;
    constexpr int AX = (MODE == 0 || MODE == 4) ? 0 : (MODE == 2 ? 2 : 1);
    const int nx = a.grid[0], ny = a.grid[1];
    const int N = a.grid[AX], pitch = N + 1;
    double2* buf = pme_lds;
    double2* tw = pme_lds + PME_FFT_TILE * pitch;
    size_t base, lstride, estride;
    int lines, first = 0;
    if (AX == 0) {
        const int total = ny * a.grid[2], l0 = (int)blockIdx.x * PME_FFT_TILE;
        lines = min(PME_FFT_TILE, total - l0);
        base = (size_t)l0 * nx; lstride = (size_t)nx; estride = 1;
    } else if (AX == 1) {
        const int tiles = (nx + PME_FFT_TILE - 1) / PME_FFT_TILE;
        const int z = (int)blockIdx.x / tiles, x0 = ((int)blockIdx.x - z * tiles) * PME_FFT_TILE;
        lines = min(PME_FFT_TILE, nx - x0);
        base = ((size_t)z * ny) * nx + x0; lstride = 1; estride = (size_t)nx;
    } else {
        const int plane = nx * ny;
        first = (int)blockIdx.x * PME_FFT_TILE;
        lines = min(PME_FFT_TILE, plane - first);
        base = (size_t)first; lstride = 1; estride = (size_t)plane;
    }
    for (int k = threadIdx.x; k < N; k += BLOCK) tw[k] = a.twiddle[AX][k];
    const int count = lines * N;
    for (int idx = threadIdx.x; idx < count; idx += BLOCK) {
        int t, j;
        if (AX == 0) { t = idx / N; j = idx - t * N; } else { j = idx / lines; t = idx - j * lines; }
        const size_t g = base + t * lstride + j * estride;
        buf[t * pitch + j] = MODE == 0 ? make_double2((double)a.charge[g] * (1.0 / PME_FIXED), 0.0) : a.work[g];
    }
    __syncthreads();
    if (MODE <= 2) pme_fft_lines<false>(buf, tw, lines, a.plan[AX], pitch);
    double e = 0.0;
    if (MODE == 2) {
        const double V = (a.box[0] * a.box[1]) * a.box[2];
        for (int idx = threadIdx.x; idx < count; idx += BLOCK) {
            const int j = idx / lines, t = idx - j * lines;
            const int p = first + t;
            const int my = p / nx, mx = p - my * nx;
            double2 F = buf[t * pitch + j];
            double G = 0.0;
            if (mx != 0 || my != 0 || j != 0) {
                const double hx = pme_fold(mx, nx) / a.box[0];
                const double hy = pme_fold(my, ny) / a.box[1];
                const double hz = pme_fold(j, N) / a.box[2];
                const double m2 = (hx * hx + hy * hy) + hz * hz;
                const double ex = exp(-((a.pi2 * m2) / a.alpha2));
                const double den = ((EW_PI * V) * m2) * ((a.modulus[0][mx] * a.modulus[1][my]) * a.modulus[2][j]);
                G = ex / den;
            }
            if (ENERGY) e = e + G * (F.x * F.x + F.y * F.y);
            buf[t * pitch + j] = make_double2(G * F.x, G * F.y);
        }
        __syncthreads();
    }
    if (MODE >= 2) pme_fft_lines<true>(buf, tw, lines, a.plan[AX], pitch);
    for (int idx = threadIdx.x; idx < count; idx += BLOCK) {
        int t, j;
        if (AX == 0) { t = idx / N; j = idx - t * N; } else { j = idx / lines; t = idx - j * lines; }
        const size_t g = base + t * lstride + j * estride;
        if (MODE == 4) a.potential[g] = buf[t * pitch + j].x;
        else a.work[g] = buf[t * pitch + j];
    }
    if (ENERGY) sum4_store(sums, a.rows, 0.5 * e, 0.0, 0.0, 0.0);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void pme_gather_kernel(const PmeArgs a) {
    const int nx = a.grid[0], ny = a.grid[1], nz = a.grid[2];
    const double* __restrict__ phi = a.potential;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const double q = a.par[3 * (size_t)i];
        if (q == 0.0) continue;
        const Vec3 x = slot_position<PREC>(a.posq, a.posq_corr, i);
        PmeAxis wx, wy, wz;
        pme_axis(x.x, a.box[0], nx, wx);
        pme_axis(x.y, a.box[1], ny, wy);
        pme_axis(x.z, a.box[2], nz, wz);
        double gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
        for (int c = 0; c < PME_ORDER; c++) {
            const size_t pz = (size_t)pme_point(wz.i0, c, nz) * ny;
#pragma unroll
            for (int b = 0; b < PME_ORDER; b++) {
                const size_t row = (pz + pme_point(wy.i0, b, ny)) * nx;
#pragma unroll
                for (int e = 0; e < PME_ORDER; e++) {
                    const double p = phi[row + pme_point(wx.i0, e, nx)];
                    gx = gx + ((wx.dth[e] * wy.th[b]) * wz.th[c]) * p;
                    gy = gy + ((wx.th[e] * wy.dth[b]) * wz.th[c]) * p;
                    gz = gz + ((wx.th[e] * wy.th[b]) * wz.dth[c]) * p;
                }
            }
        }
        const double kq = NB_COULOMB * q;
        const double fx = -((kq * ((double)nx / a.box[0])) * gx);
        const double fy = -((kq * ((double)ny / a.box[1])) * gy);
        const double fz = -((kq * ((double)nz / a.box[2])) * gz);
        Fixed3 sum;
        sum.add({fx, fy, fz});
        add_to_planes(a.force, a.padded, i, sum);
    }
}

hipError_t launch_pme(int precision, const PmeArgs& a, hipStream_t s, int stage) {
    long long points = 1;
    for (int k = 0; k < 3; k++) {
        PmeFftPlan p;
        if (!pme_fft_plan(a.grid[k], &p) || p.stages != a.plan[k].stages || p.n != a.plan[k].n || !a.twiddle[k] || !a.modulus[k]) return hipErrorInvalidValue;
        for (int r = 0; r < p.stages; r++)
            if (p.radix[r] != a.plan[k].radix[r]) return hipErrorInvalidValue;
        points *= a.grid[k];
    }
    if (a.n < 1 || points > PME_MAX_POINTS || !a.par || !a.posq || (precision == TGNH_PREC_MIXED && !a.posq_corr) || !a.charge || !a.work ||
        !a.potential || !a.force || a.padded < a.n)
        return hipErrorInvalidValue;
    const dim3 block(BLOCK);
    switch (stage) {
        case 0: TGNH_LAUNCH_PREC(pme_spread_kernel, precision, dim3(index_grid(a.n)), block, 0, s, a); break;
        case 1: TGNH_LAUNCH((pme_fft_kernel<0, false>), dim3(pme_fft_grid(a.grid, 0)), block, pme_fft_lds_bytes(a.grid[0]), s, a); break;
        case 2: TGNH_LAUNCH((pme_fft_kernel<1, false>), dim3(pme_fft_grid(a.grid, 1)), block, pme_fft_lds_bytes(a.grid[1]), s, a); break;
        case 3:
            if (a.rows) TGNH_LAUNCH((pme_fft_kernel<2, true>), dim3(pme_fft_grid(a.grid, 2)), block, pme_fft_lds_bytes(a.grid[2]), s, a);
            else TGNH_LAUNCH((pme_fft_kernel<2, false>), dim3(pme_fft_grid(a.grid, 2)), block, pme_fft_lds_bytes(a.grid[2]), s, a);
            break;
        case 4: TGNH_LAUNCH((pme_fft_kernel<3, false>), dim3(pme_fft_grid(a.grid, 1)), block, pme_fft_lds_bytes(a.grid[1]), s, a); break;
        case 5: TGNH_LAUNCH((pme_fft_kernel<4, false>), dim3(pme_fft_grid(a.grid, 0)), block, pme_fft_lds_bytes(a.grid[0]), s, a); break;
        case 6: TGNH_LAUNCH_PREC(pme_gather_kernel, precision, dim3(index_grid(a.n)), block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace tgnh
