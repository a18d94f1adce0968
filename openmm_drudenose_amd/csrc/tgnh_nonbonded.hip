// tgnh_nonbonded.hip -- the kernels behind tgnh_compute_nonbonded_force / tgnh_get_nonbonded_energy: Coulomb with a reaction field and
// Lennard-Jones between all particles inside a cutoff of a rectangular periodic box, and the exceptions, for a host that has no OpenMM
// behind it (the glue keeps OpenMM's NonbondedForce), beside the library's bonded forces (tgnh_bonded.hip).  include/drude_tgnh.h
// writes the terms one operation a line; this file follows it.  Everything in fp64 in every precision, every operation rounded on its
// own (no fused multiply-add: tests/test_nonbonded.py restates the sequence in numpy and asks for the same bits); sqrt and the
// divisions are the IEEE ones.  x(i) is slot_position's value; charges come from the table, posq.w is not read.
//
// THE CELLS, rebuilt by every call (the call is stateless: no list, no skin).  nc_d = max(1, floor(L_d / (1.001 cutoff))) cells per
// edge, formed on the host.  Four launches behind a memset of the counters:
//   nb_cell_kernel    a lane per slot: its cell from s = x / L, s -= floor(s), min((int)(s nc), nc - 1) per dimension; one integer atomic
//                     on the cell's counter (a count does not depend on the order of its increments)
//   nb_scan_kernel    one work-group: the cells' first sorted index, and the chunk table -- a cell of m members gives ceil(m / 64) chunks
//                     (cell, first sorted index), in cell order; their number is at most ncells + ceil(n / 64), the pair launch's grid
//   nb_place_kernel   a lane per slot: into its cell's run, at a cursor taken with one integer atomic -- any order within the cell
//   nb_rank_kernel    a lane per placed slot: its rank among its cell's members by counting the smaller slots, so the final order is
//                     (cell, slot) ascending whatever order the atomics gave; it writes the sorted fp64 x, y, z, q, sigma, epsilon, the
//                     slot and the slot's [lowest, highest] excluded partner
// THE PAIRS.  One wavefront per chunk; spare wavefronts leave.  A lane holds its particle and three int64 accumulators.  The distinct
// cells among c - 1, c, c + 1 per dimension (1, 2 or 3 of them) are streamed through the wavefront's own LDS image, 64 neighbours at a
// time, without a work-group barrier; every lane reads the same neighbour (a broadcast, no bank conflict).  A neighbour is excluded
// when it is the lane's own slot or, after two compares against the lane's range, a scan of the lane's list finds it.  Both lanes
// of a pair compute it (DESIGN.md 3.16 has the trade); d is exactly negated between them and everything else is symmetric, so the two
// integer shares cancel exactly.  Then one plain 64-bit load, add and store per plane into force[slot]: a slot has one lane in the
// whole launch.  No atomic touches the force buffer; no inline assembly.
// THE ENERGY (second instantiation).  A lane adds E_C and E_LJ only for neighbours whose slot is larger than its own, in traversal
// order; the rest of the order is tgnh_rows_device.h's.
// THE EXCEPTIONS.  tgnh_receiver_device.h's form: one lane per receiving slot over the table inverted at set time; no cutoff, no
// reaction field, no periodic image.
#include "tgnh_nonbonded.h"
#include "tgnh_receiver_device.h"
#include "tgnh_rows_device.h"

namespace tgnh {

#pragma clang fp contract(off)

namespace {
constexpr double NB_FIXED = 4294967296.0;

// what a wavefront has written to its LDS image is read by other lanes of the same wavefront (and the other way round)
__device__ __forceinline__ void nb_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct NbImage { double v[NB_WAVES][6][64]; int slot[NB_WAVES][64]; };      // 13 KiB a work-group; each wavefront its own

__device__ __forceinline__ int cell_coord(const double x, const double L, const int nc) {
    double s = x / L;
    s = s - floor(s);
    const int c = (int)(s * (double)nc);
    return max(0, min(c, nc - 1));                               // (a non-finite coordinate lands in some cell, inside the arrays)
}

// d - L rint(d / L), bit for bit, without the division where its result is known: |d| <= 0.49 L gives rint = 0 and d itself;
// 0.51 L <= |d| <= 1.49 L gives rint = +-1, L (+-1) = +-L exactly, and d -+ L.  (The quotient is within two ulp of |d| / L: the margins
// of 0.01 keep it off the ties at 0.5 and 1.5.)  Anything else, a NaN included, takes the header's sequence.  Five of six tested
// pairs lie outside the cutoff, and nearly all of them stop here without an fp64 division.
__device__ __forceinline__ double min_image(const double d, const double L) {
    const double ad = fabs(d);
    if (ad <= 0.49 * L) return d;
    if (ad >= 0.51 * L && ad <= 1.49 * L) return d - copysign(L, d);
    return d - L * rint(d / L);
}

template <bool ENERGY, bool EWALD = false>
__device__ __forceinline__ void pair_wave(const NonbondedArgs& a, NbImage& img, const int w, const int wave, double& e_c, double& e_lj) {
    const int lane = threadIdx.x & 63;
    const size_t n = (size_t)a.n;
    const int2 ch = a.chunks[wave];
    const int cell = ch.x, cell_end = a.cell_start[cell + 1];
    const bool active = ch.y + lane < cell_end;
    const int me = active ? ch.y + lane : ch.y;                  // (a chunk is never empty: ch.y is a member)
    const double xi = a.sorted[me], yi = a.sorted[n + me], zi = a.sorted[2 * n + me];
    const double qi = a.sorted[3 * n + me], si = a.sorted[4 * n + me], ei = a.sorted[5 * n + me];
    const int slot = a.sorted_slot[me];
    const int2 range = a.sorted_range[me];
    const int ex0 = a.excl_start[slot], ex1 = a.excl_start[slot + 1];
    long long fx = 0, fy = 0, fz = 0;
    const int c3[3] = {cell % a.nc[0], (cell / a.nc[0]) % a.nc[1], cell / (a.nc[0] * a.nc[1])};
    const int nd[3] = {min(a.nc[0], 3), min(a.nc[1], 3), min(a.nc[2], 3)};
    for (int kz = 0; kz < nd[2]; kz++) {
        const int z = (c3[2] - 1 + kz + a.nc[2]) % a.nc[2];
        for (int ky = 0; ky < nd[1]; ky++) {
            const int y = (c3[1] - 1 + ky + a.nc[1]) % a.nc[1];
            for (int kx = 0; kx < nd[0]; kx++) {
                const int x = (c3[0] - 1 + kx + a.nc[0]) % a.nc[0];
                const int other = (z * a.nc[1] + y) * a.nc[0] + x;
                const int nb1 = a.cell_start[other + 1];
                for (int base = a.cell_start[other]; base < nb1; base += 64) {
                    const int m = min(64, nb1 - base);
                    nb_wave_sync();                              // the image's last readers are done
                    if (lane < m) {
#pragma unroll
                        for (int p = 0; p < 6; p++) img.v[w][p][lane] = a.sorted[p * n + base + lane];
                        img.slot[w][lane] = a.sorted_slot[base + lane];
                    }
                    nb_wave_sync();
                    for (int k = 0; active && k < m; k++) {
                        const int js = img.slot[w][k];
                        if (js == slot) continue;
                        if (js >= range.x && js <= range.y) {
                            bool hit = false;
                            for (int e = ex0; e < ex1; e++) hit = hit || a.excl[e] == js;
                            if (hit) continue;
                        }
                        double dx = xi - img.v[w][0][k], dy = yi - img.v[w][1][k], dz = zi - img.v[w][2][k];
                        dx = min_image(dx, a.box[0]); dy = min_image(dy, a.box[1]); dz = min_image(dz, a.box[2]);
                        const double r2 = (dx * dx + dy * dy) + dz * dz;
                        if (!(r2 < a.cutoff2)) continue;
                        const double qj = img.v[w][3][k];
                        const double r = sqrt(r2), inv = 1.0 / r;
                        const double qq = NB_COULOMB * (qi * qj);     // (the product of the charges first: the same bits from both lanes, in any slot order)
                        const double sig = 0.5 * (si + img.v[w][4][k]);
                        const double e4 = 4.0 * sqrt(ei * img.v[w][5][k]);
                        const double s2 = (sig * sig) / r2;
                        const double s6 = (s2 * s2) * s2, s12 = s6 * s6;
                        double dc, ec = 0.0;
                        if (EWALD) {
                            const double ar = a.alpha * r;
                            ec = erfc(ar);
                            const double g = exp(-(ar * ar));
                            dc = qq * (-((ec * inv + a.tsp * g) * inv));
                        } else {
                            dc = qq * ((2.0 * a.krf) * r - inv * inv);
                        }
                        const double dl = (e4 * (6.0 * s6 - 12.0 * s12)) * inv;
                        const double c = -((dc + dl) * inv);
                        fx += llrint((c * dx) * NB_FIXED); fy += llrint((c * dy) * NB_FIXED); fz += llrint((c * dz) * NB_FIXED);
                        if (ENERGY && js > slot) {
                            e_c = e_c + (EWALD ? qq * (ec * inv) : qq * ((inv + a.krf * r2) - a.crf));
                            e_lj = e_lj + e4 * (s12 - s6);
                        }
                    }
                }
            }
        }
    }
    if (active) add_to_planes(a.force, a.padded, slot, {fx, fy, fz});
}
}  // namespace

template <int PREC>
__global__ __launch_bounds__(BLOCK) void nb_cell_kernel(const NonbondedArgs a) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const Vec3 x = slot_position<PREC>(a.posq, a.posq_corr, i);
        const int cell = (cell_coord(x.z, a.box[2], a.nc[2]) * a.nc[1] + cell_coord(x.y, a.box[1], a.nc[1])) * a.nc[0] + cell_coord(x.x, a.box[0], a.nc[0]);
        a.cell_of[i] = cell;
        atomicAdd(a.count + cell, 1);
    }
}

// one work-group: thread t the run of consecutive cells [t c, (t + 1) c), c = ceil(ncells / BLOCK)
__global__ __launch_bounds__(BLOCK) void nb_scan_kernel(const NonbondedArgs a) {
    __shared__ int s_members[BLOCK], s_chunks[BLOCK];
    const int per = (a.ncells + BLOCK - 1) / BLOCK;
    const int c0 = min((int)threadIdx.x * per, a.ncells), c1 = min(c0 + per, a.ncells);
    int members = 0, chunks = 0;
    for (int c = c0; c < c1; c++) { members += a.count[c]; chunks += (a.count[c] + 63) >> 6; }
    s_members[threadIdx.x] = members; s_chunks[threadIdx.x] = chunks;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = 0, k = 0;
        for (int t = 0; t < BLOCK; t++) {
            const int mt = s_members[t], kt = s_chunks[t];
            s_members[t] = m; s_chunks[t] = k;
            m += mt; k += kt;
        }
        a.cell_start[a.ncells] = m;
        *a.n_chunks = min(k, a.chunk_cap);
    }
    __syncthreads();
    members = s_members[threadIdx.x]; chunks = s_chunks[threadIdx.x];
    for (int c = c0; c < c1; c++) {
        const int m = a.count[c];
        a.cell_start[c] = members;
        for (int first = 0; first < m; first += 64, chunks++)
            if (chunks < a.chunk_cap) a.chunks[chunks] = make_int2(c, members + first);
        members += m;
    }
}

__global__ __launch_bounds__(BLOCK) void nb_place_kernel(const NonbondedArgs a) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        const int cell = a.cell_of[i];
        const int at = a.cell_start[cell] + atomicAdd(a.count + a.ncells + cell, 1);
        if (at < a.n) a.placed[at] = i;
    }
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void nb_rank_kernel(const NonbondedArgs a) {
    const size_t n = (size_t)a.n;
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < a.n; it += (long long)gridDim.x * BLOCK) {
        const int i = a.placed[(int)it];
        const int cell = a.cell_of[i];
        const int first = a.cell_start[cell], end = a.cell_start[cell + 1];
        int at = first;
        for (int p = first; p < end; p++) at += a.placed[p] < i;
        const Vec3 x = slot_position<PREC>(a.posq, a.posq_corr, i);
        a.sorted[at] = x.x; a.sorted[n + at] = x.y; a.sorted[2 * n + at] = x.z;
        a.sorted[3 * n + at] = a.par[3 * (size_t)i]; a.sorted[4 * n + at] = a.par[3 * (size_t)i + 1]; a.sorted[5 * n + at] = a.par[3 * (size_t)i + 2];
        a.sorted_slot[at] = i;
        a.sorted_range[at] = a.excl_range[i];
    }
}

__global__ __launch_bounds__(BLOCK) void nb_pair_kernel(const NonbondedArgs a) {
    __shared__ NbImage img;
    const int w = threadIdx.x >> 6, wave = blockIdx.x * NB_WAVES + w;
    double e_c = 0.0, e_lj = 0.0;
    if (wave < *a.n_chunks) pair_wave<false>(a, img, w, wave, e_c, e_lj);
}

__global__ __launch_bounds__(BLOCK) void nb_pair_energy_kernel(const NonbondedArgs a) {
    __shared__ Sum4Lds l;
    __shared__ NbImage img;
    const int w = threadIdx.x >> 6, wave = blockIdx.x * NB_WAVES + w;
    double e_c = 0.0, e_lj = 0.0;
    if (wave < *a.n_chunks) pair_wave<true>(a, img, w, wave, e_c, e_lj);
    sum4_store(l, a.rows, e_c, e_lj, 0.0, 0.0);
}

// the same two launches with Ewald summation on (tgnh_set_nonbonded_ewald): the Coulomb part of a pair is the erfc term.  The energy
// launch also leaves the two numbers of the call's box that tgnh_get_ewald_energy needs: it is the one launch every call makes
__global__ __launch_bounds__(BLOCK) void nb_pair_ewald_kernel(const NonbondedArgs a) {
    __shared__ NbImage img;
    const int w = threadIdx.x >> 6, wave = blockIdx.x * NB_WAVES + w;
    double e_c = 0.0, e_lj = 0.0;
    if (wave < *a.n_chunks) pair_wave<false, true>(a, img, w, wave, e_c, e_lj);
}

__global__ __launch_bounds__(BLOCK) void nb_pair_ewald_energy_kernel(const NonbondedArgs a) {
    __shared__ Sum4Lds l;
    __shared__ NbImage img;
    const int w = threadIdx.x >> 6, wave = blockIdx.x * NB_WAVES + w;
    double e_c = 0.0, e_lj = 0.0;
    if (wave < *a.n_chunks) pair_wave<true, true>(a, img, w, wave, e_c, e_lj);
    sum4_store(l, a.rows, e_c, e_lj, 0.0, 0.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double V = (a.box[0] * a.box[1]) * a.box[2];
        a.ew_misc[0] = -(a.bg_num / V);
        a.ew_misc[1] = (4.0 * (NB_PI * NB_COULOMB)) / V;
    }
}

// An evaluated exception (p1, p2; chargeProd, sigma, epsilon), for the receiving slot at `role`:
//   d = x(receiver) - x(other), r2 = (dx^2 + dy^2) + dz^2, r = sqrt(r2), inv = 1 / r, qq = K chargeProd, e4 = 4 epsilon,
//   s2 = (sigma sigma) / r2, s6 = (s2 s2) s2, s12 = s6 s6, dc = qq (-(inv inv)), dl = (e4 (6 s6 - 12 s12)) inv, c = -((dc + dl) inv)
template <int PREC, bool ENERGY>
__device__ __forceinline__ void exception_body(const NbExceptionArgs& a, double& e_c, double& e_lj) {
    for_each_receiver(a.recv, a.force, a.padded, [&](const int slot, const int t, const int role, Fixed3& sum) {
        const int2 at = a.atoms[t];
        const Vec3 d = slot_position<PREC>(a.posq, a.posq_corr, slot) - slot_position<PREC>(a.posq, a.posq_corr, role == 0 ? at.y : at.x);
        const double r2 = dot(d, d), rr = sqrt(r2), inv = 1.0 / rr;
        const double qq = NB_COULOMB * a.par[3 * (size_t)t], sig = a.par[3 * (size_t)t + 1], e4 = 4.0 * a.par[3 * (size_t)t + 2];
        const double s2 = (sig * sig) / r2;
        const double s6 = (s2 * s2) * s2, s12 = s6 * s6;
        const double dc = qq * (-(inv * inv));
        const double dl = (e4 * (6.0 * s6 - 12.0 * s12)) * inv;
        const double c = -((dc + dl) * inv);
        sum.add(c * d);
        if (ENERGY && role == 0) {
            e_c = e_c + qq * inv;
            e_lj = e_lj + e4 * (s12 - s6);
        }
    });
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void nb_exception_kernel(const NbExceptionArgs a) {
    double e0 = 0.0, e1 = 0.0;
    exception_body<PREC, false>(a, e0, e1);
}

template <int PREC>
__global__ __launch_bounds__(BLOCK) void nb_exception_energy_kernel(const NbExceptionArgs a) {
    __shared__ Sum4Lds l;
    double e0 = 0.0, e1 = 0.0;
    exception_body<PREC, true>(a, e0, e1);
    sum4_store(l, a.rows, e0, e1, 0.0, 0.0);
}

// pair rows [0, n_pair)[4] and exception rows [0, n_exc)[4] -> out[4].  One work-group, a thread its chunk of each (row_chunk).
__global__ __launch_bounds__(BLOCK) void nb_energy_sum_kernel(const double* __restrict__ pair_rows, const int n_pair,
                                                              const double* __restrict__ exc_rows, const int n_exc, double* __restrict__ out) {
    __shared__ Sum4Lds l;
    int r0, r1;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    row_chunk(n_pair, r0, r1);
    for (int r = r0; r < r1; r++) { s0 = s0 + pair_rows[4 * (size_t)r]; s1 = s1 + pair_rows[4 * (size_t)r + 1]; }
    row_chunk(n_exc, r0, r1);
    for (int r = r0; r < r1; r++) { s2 = s2 + exc_rows[4 * (size_t)r]; s3 = s3 + exc_rows[4 * (size_t)r + 1]; }
    sum4_put(l, s0, s1, s2, s3);
    __syncthreads();
    if (threadIdx.x < 4) out[threadIdx.x] = sum4_total(l);
}

static bool nb_args_ok(int precision, const NonbondedArgs& a) {
    return a.n >= 1 && a.par && a.excl_start && a.excl && a.excl_range && a.posq && (precision != TGNH_PREC_MIXED || a.posq_corr) &&
           a.nc[0] >= 1 && a.nc[1] >= 1 && a.nc[2] >= 1 && (long long)a.nc[0] * a.nc[1] * a.nc[2] == a.ncells && a.ncells <= NB_MAX_CELLS &&
           a.cell_of && a.count && a.cell_start && a.chunks && a.n_chunks && a.chunk_cap == nb_chunk_cap(a.n, a.ncells) && a.placed &&
           a.sorted && a.sorted_slot && a.sorted_range && a.force && a.padded >= a.n;
}

hipError_t launch_nonbonded_cells(int precision, const NonbondedArgs& a, hipStream_t s, int stage) {
    if (!nb_args_ok(precision, a)) return hipErrorInvalidValue;
    const int grid = index_grid(a.n);
    switch (stage) {
        case 0: TGNH_LAUNCH_PREC(nb_cell_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a); break;
        case 1: TGNH_LAUNCH(nb_scan_kernel, 1, BLOCK, 0, s, a); break;
        case 2: TGNH_LAUNCH(nb_place_kernel, grid, BLOCK, 0, s, a); break;
        case 3: TGNH_LAUNCH_PREC(nb_rank_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_nonbonded_pairs(int precision, const NonbondedArgs& a, hipStream_t s) {
    if (!nb_args_ok(precision, a)) return hipErrorInvalidValue;
    const int grid = nb_pair_grid(a.n, a.ncells);
    if (a.alpha > 0.0) {
        if (a.rows && !a.ew_misc) return hipErrorInvalidValue;
        if (a.rows) TGNH_LAUNCH(nb_pair_ewald_energy_kernel, grid, BLOCK, 0, s, a);
        else TGNH_LAUNCH(nb_pair_ewald_kernel, grid, BLOCK, 0, s, a);
    } else if (a.rows) TGNH_LAUNCH(nb_pair_energy_kernel, grid, BLOCK, 0, s, a);
    else TGNH_LAUNCH(nb_pair_kernel, grid, BLOCK, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_nonbonded_exceptions(int precision, const NbExceptionArgs& a, hipStream_t s) {
    if (!a.atoms || !a.par || !receivers_ok(a.recv) || !a.posq || !a.force ||
        a.padded < 1 || (precision == TGNH_PREC_MIXED && !a.posq_corr))
        return hipErrorInvalidValue;
    const int grid = index_grid(a.recv.n);
    if (a.rows) TGNH_LAUNCH_PREC(nb_exception_energy_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    else TGNH_LAUNCH_PREC(nb_exception_kernel, precision, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_nonbonded_energy_sum(const double* pair_rows, int n_pair, const double* exc_rows, int n_exc, double* out, hipStream_t s) {
    if (!pair_rows || !out || n_pair < 1 || n_exc < 0 || (n_exc > 0 && !exc_rows) || n_exc > INDEX_GRID_CAP) return hipErrorInvalidValue;
    TGNH_LAUNCH(nb_energy_sum_kernel, 1, BLOCK, 0, s, pair_rows, n_pair, exc_rows, n_exc, out);
    return hipGetLastError();
}

}  // namespace tgnh
