// tgnh_trace.h -- phase timestamps inside the kernels, tuning builds only (-DTGNH_TRACE); without it every macro here is empty.
// Included by .hip files only.
#ifndef TGNH_TRACE_H_
#define TGNH_TRACE_H_
#include "tgnh_internal.h"

namespace tgnh {
#ifdef TGNH_TRACE
// Phase timestamps of the streaming kernels (tuning builds only: tools/trace_probe.py, tools/step_trace.py).  16 slots per
// work-group, constant 100 MHz clock, written by thread 0.  One table per translation unit (static: device symbols are not
// shared between units), and so is g_chain_dbg (tgnh_chain_device.h): the readers tgnh_debug_read_trace / _clear_trace /
// _read_chain_trace / _read_chain_dbg (tgnh_kernels.hip) see what the kernels of that unit recorded -- all that record but the
// gather path's chain, whose g_chain_dbg nobody reads.
static __device__ unsigned long long g_trace[GRID_CAP * 16];
#define TRACE(slot) do { if (threadIdx.x == 0 && (slot) < 16) g_trace[blockIdx.x * 16 + (slot)] = wall_clock64(); } while (0)
#define TRACE_WAIT() __builtin_amdgcn_s_waitcnt(0)
#define TGNH_TRACE_READERS(read_name, clear_name)                                                            \
    extern "C" int read_name(unsigned long long* out) {                                                      \
        return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgnh::g_trace), sizeof(unsigned long long) * tgnh::GRID_CAP * 16); \
    }                                                                                                        \
    extern "C" int clear_name() {                                                                            \
        void* p = nullptr;                                                                                   \
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(tgnh::g_trace)) != hipSuccess) return 1;                      \
        return (int)hipMemset(p, 0, sizeof(unsigned long long) * tgnh::GRID_CAP * 16);                       \
    }
// chain_kernel's own clocks (tools/micro/chain_inside.py): wall_clock64 and clock64 at entry, after the prologue and at exit
static __device__ __attribute__((unused)) unsigned long long g_chain_trace[8];
#define CHAIN_TRACE(slot) do { if (threadIdx.x == 0) { g_chain_trace[2 * (slot)] = wall_clock64(); g_chain_trace[2 * (slot) + 1] = clock64(); } } while (0)
#else
#define TRACE(slot) do {} while (0)
#define TRACE_WAIT() do {} while (0)
#define CHAIN_TRACE(slot) do {} while (0)
#endif
}  // namespace tgnh
#endif
