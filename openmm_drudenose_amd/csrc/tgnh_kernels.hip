// tgnh_kernels.hip -- the translation unit of the DrudeTGNHIntegrator step's tiled and chain kernels (gfx950, CDNA4): their text is
// in three files by concern, compiled as ONE module.
//   tgnh_tile_kernels.h    tile_kernel, step_kernel (512-slot tiles), their dispatch and launchers
//   tgnh_wave_kernels.h    wke_kernel, wstep_kernel (wave tiles), their dispatch and launchers
//   tgnh_chain_kernels.h   chain_kernel and its siblings, rowsum_kernel, big_com_kernel, the plain kinetic-energy query
// One module, not three: what the compiler makes of the kernels that inline the Nose-Hoover chain (tile_kernel's rescale
// instantiations, chain_kernel, wstep_kernel's instantiations for chains of 2-4 links) depends on which other kernels share their
// module -- compiled apart, 37 of them come out with other control flow and register assignment from the same source (up to
// +-0.5 % instructions, more scalar registers parked in vector lanes), whatever the order of the definitions or the contraction
// pragmas; compiled together, every kernel is the code the tuning in profiles/ was done on (tools/kernel_isa.py compares two trees
// kernel by kernel).  The harness's force kernels (tgnh_harness.hip) and the gather path (tgnh_gather.hip) are units of their own.
#include "tgnh_tile_kernels.h"
#include "tgnh_wave_kernels.h"
#include "tgnh_chain_kernels.h"

#ifdef TGNH_TRACE
TGNH_TRACE_READERS(tgnh_debug_read_trace, tgnh_debug_clear_trace)
extern "C" int tgnh_debug_read_chain_trace(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgnh::g_chain_trace), sizeof(unsigned long long) * 8);
}
extern "C" int tgnh_debug_read_chain_dbg(double* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(tgnh::g_chain_dbg), sizeof(double) * 4);
}
#endif
