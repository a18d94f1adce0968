// tgnh_rescale.h -- the launchers of tgnh_rescale.hip, for the host code of tgnh_scale_velocities / tgnh_rescale_to_temperature
// (tgnh_velocities.cpp).  A header of its own, not lines of tgnh_internal.h: no header the step kernels' unit reads changes with this feature.
#ifndef TGNH_RESCALE_H_
#define TGNH_RESCALE_H_

#include "tgnh_internal.h"

namespace tgnh {

// the doubles one launch of rescale_put_kernel carries BY VALUE: what the caller's array held when the call was enqueued,
// whatever the caller does with it afterwards and however many such calls are queued behind one another (2 KiB of the 4 KiB a
// launch may carry)
constexpr int RESCALE_PUT_CHUNK = 256;
struct RescaleChunk { double v[RESCALE_PUT_CHUNK]; };
constexpr double RESCALE_INERT = -1.0;      // in a table of targets: this thermostat has no degrees of freedom (any negative value)

// dst[0 .. count) (device) = src[0 .. count) (host, read before this returns): ceil(count / 256) launches
hipError_t launch_rescale_put(double* dst, const double* src, int count, hipStream_t s);
// factors[k] = the header's rule of ke[k] and target[k], k < NT (all device): one work-group
hipError_t launch_rescale_factors(const double* ke, const double* target, int NT, double* factors, uint32_t* status, hipStream_t s);

}  // namespace tgnh

#endif
