// tgnh_drude_stats.hip -- tgnh_get_drude_statistics' two kernels: what the Drude pairs look like right now, summed on the device.
//
// The contract is the header's (include/drude_tgnh.h): per pair, in fp64 from the bound positions as they are, d2 = |x_D - x_parent|^2,
// its sum, the largest and where, how many lie beyond a threshold, a histogram of d, and the induced dipole sum q_D (x_D - x_parent).
// A read-only pass by global slot index, as the velocity draw is (tgnh_velinit.hip): thread i reads one partner word
// (partner | is-Drude << 31, -1: in no pair) and only a Drude lane goes on -- it loads its own posq (and the correction in mixed
// precision) and its parent's.  Nothing is written but one row per work-group.
//
// Same bits from any handle over the same slots: the sums are added in the fixed order of tgnh_rows_device.h, the rows by
// drude_stats_sum_kernel, one work-group.  What is counted (bins, pairs beyond the threshold, pairs) goes through integer LDS
// atomics: a count does not depend on the order.  The maximum travels as the bit pattern of d2 -- for non-negative doubles it
// orders as an unsigned 64-bit integer does -- with the slot index beside it; ties go to the lowest index.
//
// A unit of its own so that the step kernels' units compile to what they compiled to before.
#include "tgnh_rows_device.h"

namespace tgnh {

// every product and sum below is rounded on its own, as the header writes them (no fused multiply-add: a test restates them in numpy)
#pragma clang fp contract(off)

constexpr int HB = TGNH_DRUDE_HIST_BINS;
constexpr int NCOUNT = HB + 3;                  // the row's counts: HB + 1 bins, over, pairs
constexpr int NO_PAIR = 0x7fffffff;             // index beside a maximum nobody has bid for yet
static_assert(NCOUNT <= BLOCK, "one thread per count");

// what a work-group of either kernel keeps in LDS: CNT = 32-bit counts in the pass (widened in the row), 64-bit where rows are added
template <typename CNT> struct StatsLds {
    Sum4Lds sum;
    unsigned long long key;
    int idx;
    CNT count[NCOUNT];
};

template <typename CNT> __device__ __forceinline__ void stats_lds_clear(StatsLds<CNT>& l) {
    if (threadIdx.x < NCOUNT) l.count[threadIdx.x] = 0;
    if (threadIdx.x == 0) { l.key = 0ull; l.idx = NO_PAIR; }
    __syncthreads();
}

// a thread's sums, its maximum (idx == NO_PAIR: it has none) -> the work-group's row; the counts are in l.count already.
// Called as sum4_put is.
template <typename CNT>
__device__ __forceinline__ void stats_block_row(StatsLds<CNT>& l, double s0, double s1, double s2, double s3,
                                                const unsigned long long key, const int idx, DrudeStatsRow* __restrict__ row) {
    sum4_put(l.sum, s0, s1, s2, s3);
    if (idx != NO_PAIR) atomicMax(&l.key, key);
    __syncthreads();
    if (idx != NO_PAIR && key == l.key) atomicMin(&l.idx, idx);        // ties: the lowest index
    __syncthreads();
    if (threadIdx.x < 4) (threadIdx.x == 0 ? row->sum_d2 : row->dipole[threadIdx.x - 1]) = sum4_total(l.sum);
    if (threadIdx.x < HB + 1) row->hist[threadIdx.x] = (long long)l.count[threadIdx.x];
    if (threadIdx.x == HB + 1) row->over = (long long)l.count[HB + 1];
    if (threadIdx.x == HB + 2) row->pairs = (long long)l.count[HB + 2];
    if (threadIdx.x == 0) { row->max_key = l.key; row->worst = l.idx; row->pad = 0; }
}

template <int PREC>
__device__ __forceinline__ void load_site(const typename Prec<PREC>::real4* __restrict__ posq, const float4* __restrict__ corr, const int i,
                                          double& x, double& y, double& z, double& q) {
    const typename Prec<PREC>::real4 p = posq[i];
    x = (double)p.x; y = (double)p.y; z = (double)p.z; q = (double)p.w;
    if (PREC == TGNH_PREC_MIXED) {
        const float4 c = corr[i];
        x = x + (double)c.x; y = y + (double)c.y; z = z + (double)c.z;
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void drude_stats_kernel(const typename Prec<PREC>::real4* __restrict__ posq, const float4* __restrict__ corr,
                                                            const int* __restrict__ partner, const int n, const double thr2,
                                                            const double hist_max, DrudeStatsRow* __restrict__ rows) {
    __shared__ StatsLds<unsigned int> l;
    stats_lds_clear(l);
    double s_d2 = 0.0, px = 0.0, py = 0.0, pz = 0.0;
    unsigned long long best = 0ull;
    int best_i = NO_PAIR;
    unsigned int over = 0, pairs = 0;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const int pj = partner[i];
        if (pj >= -1) continue;                                  // in no pair (-1), or a parent: its Drude lane does the pair
        const int j = pj & 0x7fffffff;                           // (inside [0, n): the table is built from the pair lists tgnh_create checked)
        double xd, yd, zd, qd, xp, yp, zp, qp;
        load_site<PREC>(posq, corr, i, xd, yd, zd, qd);
        load_site<PREC>(posq, corr, j, xp, yp, zp, qp);
        const double dx = xd - xp, dy = yd - yp, dz = zd - zp;
        const double d2 = dx * dx + dy * dy + dz * dz;
        s_d2 = s_d2 + d2;
        px = px + qd * dx; py = py + qd * dy; pz = pz + qd * dz;
        pairs++;
        if (d2 > thr2) over++;
        const unsigned long long key = (unsigned long long)__double_as_longlong(d2);
        if (best_i == NO_PAIR || key > best) { best = key; best_i = i; }     // (a thread's indices ascend: the first of equals stays)
        if (hist_max > 0.0) {
            const double qn = sqrt(d2) * (double)HB / hist_max;
            int k = qn >= (double)HB ? HB : (int)qn;             // (a NaN position: neither branch means anything; the clamp keeps the index inside the bins)
            k = min(max(k, 0), HB);
            atomicAdd(&l.count[k], 1u);
        }
    }
    if (over) atomicAdd(&l.count[HB + 1], over);
    if (pairs) atomicAdd(&l.count[HB + 2], pairs);
    stats_block_row(l, s_d2, px, py, pz, best, best_i, rows + blockIdx.x);
}

// rows [0, nrows) -> *out.  One work-group, a thread its chunk of the rows (row_chunk).
__global__ __launch_bounds__(BLOCK) void drude_stats_sum_kernel(const DrudeStatsRow* __restrict__ rows, const int nrows, DrudeStatsRow* __restrict__ out) {
    __shared__ StatsLds<unsigned long long> l;
    stats_lds_clear(l);
    int r0, r1;
    row_chunk(nrows, r0, r1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    unsigned long long best = 0ull;
    int best_i = NO_PAIR;
    for (int r = r0; r < r1; r++) {
        const DrudeStatsRow& w = rows[r];
        s0 = s0 + w.sum_d2; s1 = s1 + w.dipole[0]; s2 = s2 + w.dipole[1]; s3 = s3 + w.dipole[2];
        if (w.worst != NO_PAIR && (best_i == NO_PAIR || w.max_key > best || (w.max_key == best && w.worst < best_i))) { best = w.max_key; best_i = w.worst; }
        if (w.pairs) {                                           // (a row without a pair has no count either)
            for (int k = 0; k < HB + 1; k++)
                if (w.hist[k]) atomicAdd(&l.count[k], (unsigned long long)w.hist[k]);
            if (w.over) atomicAdd(&l.count[HB + 1], (unsigned long long)w.over);
            atomicAdd(&l.count[HB + 2], (unsigned long long)w.pairs);
        }
    }
    stats_block_row(l, s0, s1, s2, s3, best, best_i, out);
}

hipError_t launch_drude_stats(int precision, const void* posq, const void* posq_corr, const int* partner, int n, double threshold,
                              double hist_max, DrudeStatsRow* rows, int grid, hipStream_t s) {
    if (n < 1 || grid < 1 || grid > INDEX_GRID_CAP) return hipErrorInvalidValue;
    const double thr2 = threshold * threshold;
    const float4* corr = static_cast<const float4*>(posq_corr);
    switch (precision) {
        case TGNH_PREC_SINGLE:
            TGNH_LAUNCH(drude_stats_kernel<TGNH_PREC_SINGLE>, grid, BLOCK, 0, s, static_cast<const float4*>(posq), corr, partner, n, thr2, hist_max, rows); break;
        case TGNH_PREC_MIXED:
            if (!corr) return hipErrorInvalidValue;
            TGNH_LAUNCH(drude_stats_kernel<TGNH_PREC_MIXED>, grid, BLOCK, 0, s, static_cast<const float4*>(posq), corr, partner, n, thr2, hist_max, rows); break;
        case TGNH_PREC_DOUBLE:
            TGNH_LAUNCH(drude_stats_kernel<TGNH_PREC_DOUBLE>, grid, BLOCK, 0, s, static_cast<const double4*>(posq), corr, partner, n, thr2, hist_max, rows); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(drude_stats_sum_kernel, 1, BLOCK, 0, s, rows, grid, rows + grid);
    return hipGetLastError();
}

}  // namespace tgnh
