// tgnh_meet_device.h -- the meeting of the one-launch step kernels (step_kernel, wstep_kernel), between their two passes.
// Included by .hip files only.
#ifndef TGNH_MEET_DEVICE_H_
#define TGNH_MEET_DEVICE_H_
#include "tgnh_tile_device.h"
#include "tgnh_chain_device.h"
#include "tgnh_slot_device.h"

namespace tgnh {

// The meeting of step_kernel / wstep_kernel: every work-group hands in its row of kinetic-energy sums (tagged cells), work-group 0
// collects them in a fixed order and sends the sums to the mailbox of every rank, one wavefront of every work-group waits for all
// ranks' sums and runs both chain halves (the scale factors land in sh.s_scale).  `prefetch` is called between handing in the
// row and the wait: the loads the second pass will need.  Returns false when an exchange timed out (nothing may be stored).
struct MeetShared {
    double* s_scale;                                  // [MAX_GROUPS + 2]
    double (*s_part)[CHAIN_INLINE_SUM_NT];            // [TBLOCK / 64]
    double* s_x;                                      // [64 + XCHG_MAX_WORLD * CHAIN_INLINE_SUM_NT]
    int* s_go_p; unsigned* s_gen_p; unsigned long long* s_seq1_p;
    const double* s_block;                            // MULTI: the thermostat block as it was at kernel entry (chains of 2-4 links)
};
template <int PREC, int GB, bool LEAN = false, int NTH = TBLOCK, bool MULTI = false, typename Prefetch>
__device__ __forceinline__ bool step_meet(const TileArgs& a, TileEnv<PREC, GB>& e, const unsigned gen0, const unsigned long long seq0,
                                          Chain1Regs& creg, const MeetShared& sh, Prefetch&& prefetch) {
    double* const s_scale = sh.s_scale; double (*const s_part)[CHAIN_INLINE_SUM_NT] = sh.s_part; double* const s_x = sh.s_x;
    int& s_go = *sh.s_go_p; unsigned& s_gen = *sh.s_gen_p; unsigned long long& s_seq1 = *sh.s_seq1_p;
    const int tid = threadIdx.x, G = a.num_groups, NT = G + 2, grid = (int)gridDim.x;
    const bool chain_wave = tid < 64, leader = blockIdx.x == 0;
    const int itg = tid & 63;
    const ChainLayout& L = a.chain.L;
    // the thermostat block has been read (its values are in registers) before this work-group's row is stored
    if (chain_wave) asm volatile("" :: "v"(creg.eta), "v"(creg.etaDot0), "v"(creg.etaDot1), "v"(creg.etaDotDot), "v"(creg.etaMass), "v"(creg.nkbt) : "memory");
    ke_reduce<PREC, GB, true, NTH>(a, e, gen0 + 1u, s_x);
    TRACE(2);
    // what the second pass needs of the held tile beyond what is in registers (its positions): issued now, needed after the meeting
    prefetch();
    // ... and what the chain can form without the sums (index map, constants, 1/Q, expfac): done while the others still work
    // (single precision: its 16 registers there would cost the kernel its fourth work-group per compute unit)
    constexpr bool EARLY_PRE = PREC != TGNH_PREC_SINGLE && !LEAN;      // (LEAN: wstep_kernel, which lives on a small register count: with it 130 VGPRs, one work-group per compute unit)
    Chain1Pre cpre{};
    if (EARLY_PRE && chain_wave && !L.c1_quirk && !(MULTI && L.C > 1)) cpre = chain1_prepare(a.chain, creg, itg);

    // ---- meet: work-group 0 collects the rows.  Thread t owns rows t, t + 256, ...: it polls their cells until all
    // carry this launch's tag and adds them in row order; then 64-lane sums and one LDS hop, fixed order throughout.
    if (tid == 0) { s_gen = gen0; s_seq1 = seq0 + 1ull; }
    __syncthreads();
    const unsigned long long want = (unsigned long long)(s_gen + 1u);
    if (leader) {
        unsigned long long* const my_peer = xchg_peer_of(a.chain.x, tid);   // for the send: fetched before the collection, not after
        constexpr int NTM = GB + 2;                        // NT = G + 2 <= GB + 2: the register arrays follow the instantiation
        double acc[NTM];
#pragma unroll
        for (int b = 0; b < NTM; b++) acc[b] = 0.0;
        bool ok = true;
        TRACE(6);
        ok = collect_rows<GB, LEAN, NTH>(a, tid, grid, NT, want, acc);
        TRACE(10);
        if (!ok) {                                         // a work-group never handed in its row: nobody goes on (no send below)
            atomicOr(a.status, 8u);
            __hip_atomic_store(a.chain.x.dead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const double* big = a.partials + (size_t)GRID_CAP * NT;               // rows of big_com_kernel (an earlier launch)
        for (int r = tid; r < a.chain.nbig; r += NTH)
#pragma unroll
            for (int b = 0; b < NTM; b++) if (b < NT) acc[b] += big[(size_t)r * NT + b];
#pragma unroll
        for (int b = 0; b < NTM; b++) {
            if (b < NT) {
                const double t = wave_sum(acc[b]);
                if ((tid & 63) == 0) s_part[tid >> 6][b] = t;
            }
        }
        // (the barrier of the hand-over doubles as the vote: one thread that gave up on a row stops the whole send -- incomplete
        // sums under a valid tag would let every waiter, here and on the peer ranks, integrate with wrong scale factors; without
        // the send they time out or see the latch, and nothing is stored)
        const bool all_ok = __syncthreads_and(ok ? 1 : 0) != 0;
        TRACE(7);
        // the send (xchg_send's stores, tgnh_xchg_device.h), straight from the four wavefronts' partial sums: every storing
        // thread adds them itself, in wavefront order -- no second hand-over through LDS, no second barrier on this path
        const XchgArgs& x = a.chain.x;
        const unsigned long long seq = s_seq1, stag = (seq & 0xffffffffull) << 32;
        if (tid == 0) { a.sync[1] = s_gen + 1u; *x.seq = seq; }      // the next launch's rows carry the next tag
        const int tpp = NTH / x.world;
        if (all_ok && tid < tpp * x.world) {
            unsigned long long* const base = my_peer + xchg_cell(x, (unsigned)(seq & 1ull), x.rank, 0, 0);
            for (int q = tid / x.world; q < NT * XCHG_REPLICAS; q += tpp) {
                const int copy = q / NT, i = q - copy * NT;
                double v = 0.0;
#pragma unroll
                for (int w = 0; w < NTH / 64; w++) v += s_part[w][i];
                unsigned long long* cell = base + (size_t)copy * XCHG_REPLICA_U64 + (size_t)i * XCHG_CELL_U64;
                store_tagged(cell, cell + 1, stag, v);
            }
        }
        TRACE(13);
    }
    if (chain_wave) {
        bool dead = false;                                 // an exchange has timed out, now or earlier (the latch)
        const double mine = xchg_wait_sum<true>(a.chain.x, NT, itg, s_x + 64, seq0 + 1ull, &dead);
        TRACE(8);
        if (itg == 0) s_go = dead ? 0 : 1;
        if (!dead) {
            const bool write = leader;
            creg.ke = mine;
            if (write && itg < NT) a.st_out[L.off_ke_red + itg] = mine;
            if (write) {                                   // Cu :493-497 (work-group 0 only: the others go straight on to the chain)
                const double kesum = wave_sum(itg < NT ? mine : 0.0);
                if (itg == 63) a.st_out[L.off_kesum] = 0.5 * kesum;
            }
            if (MULTI && L.C > 1) chainN_run<false>(a.chain, sh.s_block, a.st_out, write, s_scale, itg, mine);
            else if (itg < NT) {
                if (L.c1_quirk) chain1q_run(a.chain, creg, a.st_out, write, s_scale, itg);
                else chain1_finish(a.chain, creg, EARLY_PRE ? cpre : chain1_prepare(a.chain, creg, itg), a.st_out, write, s_scale, itg);
            }
        }
    }
    __syncthreads();
    return s_go != 0;
}

}  // namespace tgnh
#endif
