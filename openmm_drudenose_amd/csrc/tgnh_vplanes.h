// tgnh_vplanes.h -- the launchers of tgnh_vplanes.hip, for the host code of the one-launch step (tgnh_step.cpp): the two layout
// conversions between the caller's velm and the library's own velocity planes.  A header of its own, as tgnh_rescale.h is.
#ifndef TGNH_VPLANES_H_
#define TGNH_VPLANES_H_

#include "tgnh_internal.h"

namespace tgnh {

// planes[c * stride + word(i)] = velm[i].{x, y, z}, i over the MASSIVE slots of the wave tiles wave_tile[0 .. num_wtiles] (device
// copy: y carries period | pattern << 8 in its high bits); word(i) = wtile_base[tile] + wpat_off[pattern * PATTERN_WORDS + lane],
// massive = the slot's entry of wpat_invm (Prec::mixed [patterns][PATTERN_WORDS]) is not 0.  mismatch != nullptr: every slot's w
// is compared, bit for bit, with that entry; a slot that differs, a tile without a pattern, or a massless slot whose x, y or z is
// not finite ORs 1 into *mismatch.
hipError_t launch_velm_to_planes(int precision, const void* velm, void* planes, const int2* wave_tile, int num_wtiles,
                                 const void* wpat_invm, const uint32_t* wtile_base, const uint32_t* wpat_off, int stride,
                                 uint32_t* mismatch, hipStream_t s);
// velm[i] = (planes x, y, z of slot i, velm[i].w as read) for the massive slots; a massless slot of velm is not touched
hipError_t launch_planes_to_velm(int precision, const void* planes, void* velm, const int2* wave_tile, int num_wtiles,
                                 const void* wpat_invm, const uint32_t* wtile_base, const uint32_t* wpat_off, int stride, hipStream_t s);

}  // namespace tgnh

#endif
