// tgnh_virtual_sites.h -- the launchers of tgnh_virtual_sites.hip, for the host code of tgnh_compute_virtual_sites /
// tgnh_distribute_virtual_site_forces (tgnh_virtual_sites.cpp).  A header of its own, as tgnh_constraints.h is: no header the step
// kernels' unit reads changes with this feature.
#ifndef TGNH_VIRTUAL_SITES_H_
#define TGNH_VIRTUAL_SITES_H_

#include "tgnh_internal.h"
#include "tgnh_receivers.h"

namespace tgnh {

enum : int { VS_TWO_AVERAGE = 0, VS_THREE_AVERAGE = 1, VS_OUT_OF_PLANE = 2, VS_LOCAL_COORDINATES = 3, VS_KINDS = 4 };   // include/drude_tgnh.h: TGNH_SITE_*
constexpr int VS_PARAMS = 12;                // parameters per site as the caller hands them over, and planes of SiteTable::params
constexpr int VS_PARAMS_USED[VS_KINDS] = {2, 3, 3, 12};

// The site table, one entry per site in each array (lane c reads entry c of every array), rows sorted by the site's slot.
struct SiteTable {
    const int4* atoms;        // [n] (site, p1, p2, p3); p3 = -1 for a two-particle site
    const int* kind;          // [n] VS_*
    const double* params;     // [VS_PARAMS][n] planes, in the order of include/drude_tgnh.h; what a kind does not use holds the host's zero
    int n;                    // (every index of `atoms` but a -1 is a slot of the bound arrays: the host checked at set time)
};

struct SitePlaceArgs {
    SiteTable t;
    void* posq; void* posq_corr;
};

// The table and its inverse (tgnh_receivers.h): a term is a row of the table, a role 0, 1, 2 for p1, p2, p3 of that row.
struct SiteSpreadArgs {
    SiteTable t;
    ReceiverTable recv;
    const void* posq; const void* posq_corr;
    long long* force;         // [3 * padded] fixed point x 2^32, planes x | y | z
    int padded;
};

inline int vs_grid(int n) { return (int)(((long long)n + BLOCK - 1) / BLOCK); }   // one lane per row (cn_grid's rule): no grid-stride loop, no cap

hipError_t launch_place_sites(int precision, const SitePlaceArgs& a, hipStream_t s);
hipError_t launch_spread_site_forces(int precision, const SiteSpreadArgs& a, hipStream_t s);

}  // namespace tgnh

#endif
