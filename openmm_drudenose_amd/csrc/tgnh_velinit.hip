// tgnh_velinit.hip -- tgnh_set_velocities_to_temperature's one kernel: Drude-aware starting velocities, drawn on the device.
//
// The contract is the header's (include/drude_tgnh.h): a pair's centre of mass at T, its relative motion at T_D, every other
// massive slot at T, massless slots 0; normals from Philox4x32-10 keyed by the seed and counted by the GLOBAL slot index, so a
// slot's velocity is a function of (seed, global index, the masses of its pair) and of nothing else -- not of the tiling, the
// step path, the grid or the sharding.  One kernel by global index therefore serves every handle: thread i owns slot i, asks
// for its own velm[i] before it knows the slot's role (tgnh_gather.hip's habit), reads one partner word
// (partner | is-Drude << 31, -1: in no pair), and for a pair member loads the partner's w, forms BOTH draws of the pair (two
// Philox calls) and stores its own slot only: a wavefront's stores are consecutive, no scatter, no atomic, no LDS.  A
// once-per-run launch: per slot it reads and writes velm once, reads 4 B of index and gathers the partner's w.
//
// A unit of its own so that the step kernels' units compile to what they compiled to before.
#include <algorithm>

#include "tgnh_by_index.h"

namespace tgnh {

struct Philox4 { uint32_t x0, x1, x2, x3; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

// z(gi): three standard normals of global index gi (Box-Muller on the four words, the fourth normal discarded)
__device__ __forceinline__ void normals3(const unsigned long long seed, const unsigned long long gi, double& zx, double& zy, double& zz) {
    const Philox4 x = philox4x32_10((uint32_t)gi, (uint32_t)(gi >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double two32inv = 2.3283064365386963e-10;              // 2^-32: u in (0, 1), exact in fp64
    const double u0 = ((double)x.x0 + 0.5) * two32inv, u1 = ((double)x.x1 + 0.5) * two32inv;
    const double u2 = ((double)x.x2 + 0.5) * two32inv, u3 = ((double)x.x3 + 0.5) * two32inv;
    const double twopi = 6.283185307179586;
    const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
    zx = r0 * cos(twopi * u1); zy = r0 * sin(twopi * u1); zz = r1 * cos(twopi * u3);
}

template <typename V4, typename T>
__global__ __launch_bounds__(BLOCK) void velinit_kernel(V4* __restrict__ velm, const int* __restrict__ partner, const int n,
                                                        const double kT, const double kTD, const unsigned long long seed,
                                                        const unsigned long long first) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < n; it += (long long)gridDim.x * BLOCK) {
        const int i = (int)it;
        V4 v = velm[i];                                          // own data first: no load of it waits for the partner word
        const int pj = partner[i];
        double vx = 0.0, vy = 0.0, vz = 0.0;
        if (v.w != 0) {
            const double m = 1.0 / (double)v.w;
            if (pj == -1) {
                double zx, zy, zz;
                normals3(seed, first + (unsigned long long)i, zx, zy, zz);
                const double s = sqrt(kT / m);
                vx = s * zx; vy = s * zy; vz = s * zz;
            } else {
                const int j = pj & 0x7fffffff;                   // (inside [0, n): the table is built from the pair lists tgnh_create checked)
                const bool drude = pj < 0;
                const double mo = 1.0 / (double)velm[j].w;       // (a pair has no massless member: refused at create)
                const double m_d = drude ? m : mo, m_p = drude ? mo : m;
                const double mt = m_d + m_p, mu = m_d * m_p / mt;
                double cx, cy, cz, rx, ry, rz;
                normals3(seed, first + (unsigned long long)(drude ? j : i), cx, cy, cz);     // z(parent): the centre of mass
                normals3(seed, first + (unsigned long long)(drude ? i : j), rx, ry, rz);     // z(Drude): v_rel = v_parent - v_drude
                const double sc = sqrt(kT / mt), sr = sqrt(kTD / mu);
                const double f = drude ? -(m_p / mt) : m_d / mt;
                vx = sc * cx + (sr * rx) * f; vy = sc * cy + (sr * ry) * f; vz = sc * cz + (sr * rz) * f;
            }
        }
        v.x = (T)(vx + 0.0); v.y = (T)(vy + 0.0); v.z = (T)(vz + 0.0);      // (+ 0.0: T = 0 stores +0, not the sign of a normal)
        velm[i] = v;                                             // w goes back as it came
    }
}

hipError_t launch_velinit(int precision, void* velm, const int* partner, int n, double kT, double kTD,
                          unsigned long long seed, long long first_particle, hipStream_t s) {
    if (n < 1) return hipSuccess;
    const int grid = (int)std::min<long long>(((long long)n + BLOCK - 1) / BLOCK, 8192);
    if (precision == TGNH_PREC_SINGLE)
        velinit_kernel<float4, float><<<grid, BLOCK, 0, s>>>(static_cast<float4*>(velm), partner, n, kT, kTD, seed, (unsigned long long)first_particle);
    else
        velinit_kernel<double4, double><<<grid, BLOCK, 0, s>>>(static_cast<double4*>(velm), partner, n, kT, kTD, seed, (unsigned long long)first_particle);
    return hipGetLastError();
}

}  // namespace tgnh
