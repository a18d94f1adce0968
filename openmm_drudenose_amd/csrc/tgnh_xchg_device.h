// tgnh_xchg_device.h -- how work-groups and ranks hand sums to each other without read-modify-write atomics: tagged 8-byte cells
// (data and "it is there" in one store).  The mailbox exchange between ranks (protocol: XchgArgs in tgnh_internal.h) and the
// tagged rows work-group 0 collects inside a launch.  Included by .hip files only.
#ifndef TGNH_XCHG_DEVICE_H_
#define TGNH_XCHG_DEVICE_H_
#include "tgnh_device_math.h"

namespace tgnh {

// ---- mailbox exchange (protocol: XchgArgs in tgnh_internal.h) ----
__device__ __forceinline__ size_t xchg_cell(const XchgArgs& x, const unsigned par, const int src, const int i, const int copy = 0) {
    return (size_t)copy * XCHG_REPLICA_U64 + (((size_t)par * x.world + src) * XCHG_NT_PAD + i) * XCHG_CELL_U64;
}
__device__ __forceinline__ unsigned long long xchg_ld(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// A tagged cell: a double as two 8-byte words {32 bits of it, tag} -- data and "it is there" in one atomic store each.
// tag: already in the upper half.
__device__ __forceinline__ void store_tagged(unsigned long long* lo, unsigned long long* hi, const unsigned long long tag, const double v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    __hip_atomic_store(lo, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hi, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The mailbox thread tid of a sending work-group stores into: thread tid serves peer tid % world, so every thread needs ONE
// mailbox pointer, which a caller with time to spare fetches ahead of the send (step_kernel: before it collects the rows).
__device__ __forceinline__ unsigned long long* xchg_peer_of(const XchgArgs& x, const int tid) {
    return x.world == 1 ? x.mine : x.peers[tid % x.world];
}
// Called by one work-group with `mine` = this rank's sum in thread tid < NT, handed over through s_val (LDS, NT doubles).
// Contains __syncthreads().  seq_new != 0 (thread 0): the number of this exchange, when the caller has read the counter
// already (step_kernel reads it at kernel entry: no load on the path between the last row and the send).
// peer = xchg_peer_of(x, tid) when the caller has fetched it already.
__device__ __forceinline__ void xchg_send(const XchgArgs& x, const int NT, const int tid, const int nthreads, double* s_val,
                                          const double mine, const unsigned long long seq_new = 0ull,
                                          unsigned long long* peer = nullptr) {
    __shared__ unsigned long long s_seq;
    if (!peer) peer = xchg_peer_of(x, tid);
    if (tid == 0) { const unsigned long long s = seq_new ? seq_new : *x.seq + 1ull; *x.seq = s; s_seq = s; }
    if (tid < NT) s_val[tid] = mine;
    __syncthreads();
    const unsigned long long seq = s_seq, tag = (seq & 0xffffffffull) << 32;
    const int tpp = nthreads / x.world;                      // threads per peer
    if (tid >= tpp * x.world) return;
    // every copy of the peer's cells [parity][my rank][0 .. NT): copy-major, so copy 0 goes out first
    unsigned long long* const base = peer + xchg_cell(x, (unsigned)(seq & 1ull), x.rank, 0, 0);
    for (int q = tid / x.world; q < NT * XCHG_REPLICAS; q += tpp) {
        const int copy = q / NT, i = q - copy * NT;
        const double v = s_val[i];                           // (read before the cell's address is formed: the order the registers follow)
        unsigned long long* cell = base + (size_t)copy * XCHG_REPLICA_U64 + (size_t)i * XCHG_CELL_U64;
        store_tagged(cell, cell + 1, tag, v);
    }
}
// Called by all 64 lanes of one wavefront, converged; s_val = LDS scratch of world*NT doubles owned by that wavefront.
// Returns the all-rank sum of thermostat `lane` (lanes < NT).  seq_expected != 0: the exchange to wait for when this
// rank's own send may not have happened yet (step_kernel: sender and waiters are work-groups of one launch).
// SPREAD: the work-groups of the launch poll different copies of the cells (step_kernel, where all of them wait at the
// same moment); otherwise copy 0.
template <bool SPREAD = false>
__device__ __forceinline__ double xchg_wait_sum(const XchgArgs& x, const int NT, const int lane, double* s_val,
                                                const unsigned long long seq_expected = 0ull, bool* failed = nullptr) {
    const int cells = x.world * NT;
    const bool stamp = x.stat != nullptr && blockIdx.x == 0;            // work-group 0 keeps the rank's wait statistics
    const unsigned long long t_in = stamp ? wall_clock64() : 0ull;
    const unsigned long long* const box = x.mine + (SPREAD ? (size_t)(blockIdx.x % (unsigned)XCHG_REPLICAS) * XCHG_REPLICA_U64 : 0);
    // first batch: counter, latch and both parities of this lane's first cell, all in flight together
    const unsigned long long seq_raw = seq_expected ? seq_expected : __hip_atomic_load(x.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned dead = __hip_atomic_load(x.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (lane < cells) {
        const int r = lane / NT, i = lane - r * NT;
        const unsigned long long* c0 = box + xchg_cell(x, 0u, r, i);
        const unsigned long long* c1 = box + xchg_cell(x, 1u, r, i);
        a0 = xchg_ld(c0); a1 = xchg_ld(c0 + 1); b0 = xchg_ld(c1); b1 = xchg_ld(c1 + 1);
    }
    const unsigned par = (unsigned)(seq_raw & 1ull);
    const unsigned long long tag = seq_raw & 0xffffffffull;
    bool timed_out = false;
    for (int k = lane; k < cells; k += 64) {
        const int r = k / NT, i = k - r * NT;
        const unsigned long long* c = box + xchg_cell(x, par, r, i);
        unsigned long long w0, w1;
        if (k == lane) { w0 = par ? b0 : a0; w1 = par ? b1 : a1; }
        else { w0 = xchg_ld(c); w1 = xchg_ld(c + 1); }
        unsigned n = 0;
        while (((w0 >> 32) != tag || (w1 >> 32) != tag) && dead == 0u && !timed_out) {
            if (++n > XCHG_SPIN_LIMIT) { timed_out = true; break; }
            // the latch may be set while this wavefront is already polling (step_kernel's work-group 0 giving up on a row, another
            // wavefront's time-out): looked at again every 64 polls, so that a failure ends every wait within microseconds
            if ((n & 63u) == 0u) dead = __hip_atomic_load(x.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_s_sleep(4);
            w0 = xchg_ld(c); w1 = xchg_ld(c + 1);
        }
        s_val[k] = __longlong_as_double((long long)((w1 << 32) | (w0 & 0xffffffffull)));
    }
    if (timed_out) {
        atomicOr(x.status, 4u);
        __hip_atomic_store(x.dead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (failed) *failed = __any(timed_out || dead != 0u);
    if (stamp) {                                                        // from "my sums are out" to "everybody's are here"
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long dt = wall_clock64() - t_in;
        if (lane == 0) {                                                // (one writer per launch: plain read-modify-write)
            x.stat[0] += dt;
            if (dt > x.stat[1]) x.stat[1] = dt;
            x.stat[2] += 1ull;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double s = 0.0;
    if (lane < NT)
        for (int r = 0; r < x.world; r++) s += s_val[r * NT + lane];       // rank order, on every rank
    return s;
}

// step_kernel's tagged rows: word j (two per thermostat) of row r.  Rows come in blocks of 64 -- the rows one wavefront of the
// collecting work-group reads with one load -- and inside a block word-major: the 64 lanes of a load read 512 contiguous
// bytes (one request per 64-byte line instead of one per lane: the collection is bound by the requests a single compute
// unit issues), and the words of a row lie 512 bytes apart, within reach of a load's immediate offset (one address per row).
__device__ __forceinline__ size_t row_word(const int r, const int j) {
    return ((size_t)(r >> 6) * (2 * CHAIN_INLINE_SUM_NT) + j) * 64 + (r & 63);
}

// Work-group 0 collects the tagged rows of a launch (ke_reduce<TAGGED>): thread t owns rows t, t + NTH, ...: it polls their cells
// until all carry `want` and adds them in row order into acc[] (fixed order: reproducible bits).  Returns false when a row
// never came (bounded polling).
template <int GB, bool LEAN, int NTH>
__device__ __forceinline__ bool collect_rows(const TileArgs& a, const int tid, const int grid, const int NT, const unsigned long long want,
                                             double (&acc)[GB + 2]) {
    constexpr int NTM = GB + 2;
    bool ok = true;
    // RB rows of this thread per batch of loads (all of them for the resident grid of 768 when G = 1): once the last row
        // is there, one more round trip sees everything -- polled row after row, a thread whose first row came last paid
        // a round trip for each of the others behind it.  CH thermostats of a row per batch: the registers a batch takes
        // (2 x CH x RB words) do not grow with the number of temperature groups.  A row seen complete is not read again: a
        // round waits for all of its loads together (~1 us with everything polled), and the round that finally sees the last
        // row is a short one when it polls the stragglers only (last row -> all seen 1.6 instead of 2.3 us at 625 k slots).
        constexpr int RB = (GB == 1 && !LEAN) ? 3 : 1, CH = 3;
#pragma unroll 1
        for (int r0 = tid; r0 < grid && ok; r0 += RB * NTH) {
#pragma unroll 1
            for (int b0 = 0; b0 < NT && ok; b0 += CH) {
                unsigned long long w[RB][2 * CH];
                bool have[RB];                              // a row seen complete is not read again: later rounds poll the stragglers only
#pragma unroll
                for (int k = 0; k < RB; k++) have[k] = r0 + k * NTH >= grid;
                unsigned n = 0;
                for (;;) {
#pragma unroll
                    for (int k = 0; k < RB; k++) {
                        if (!have[k]) {
                            const unsigned long long* cell = a.rows + row_word(r0 + k * NTH, 2 * b0);   // the lanes of a load read consecutive words
#pragma unroll
                            for (int b = 0; b < 2 * CH; b++) if (b0 + b / 2 < NT) w[k][b] = xchg_ld(cell + b * 64);
                        }
                    }
                    bool all = true;
#pragma unroll
                    for (int k = 0; k < RB; k++) {
                        if (!have[k]) {
                            bool row = true;
#pragma unroll
                            for (int b = 0; b < 2 * CH; b++) if (b0 + b / 2 < NT) row = row && (w[k][b] >> 32) == want;
                            have[k] = row;
                        }
                        all = all && have[k];
                    }
                    if (all) break;
                    if (++n > XCHG_SPIN_LIMIT) { ok = false; break; }
                }
#pragma unroll
                for (int k = 0; k < RB; k++)                // row order: r0, r0 + 256, ...
#pragma unroll
                    for (int b = 0; b < CH; b++)
                        if (b0 + b < NT && r0 + k * NTH < grid) {
                            const double v = __longlong_as_double((long long)((w[k][2 * b + 1] << 32) | (w[k][2 * b] & 0xffffffffull)));
#pragma unroll
                            for (int t = 0; t < NTM; t++) acc[t] += (t == b0 + b) ? v : 0.0;
                        }
            }
        }
    return ok;
}

}  // namespace tgnh
#endif
