// tgnh_receiver_device.h -- what a lane does with a table of receiving slots (tgnh_receivers.h), written once for the library's
// forces (tgnh_virtual_sites.hip, tgnh_drude_force.hip, tgnh_bonded.hip, tgnh_nonbonded.hip).  Included by .hip files only.
//
// THE FORM.  One lane per RECEIVING slot, a grid-stride loop over the receivers in index_grid's grid.  A lane walks its slot's list;
// per entry (term, role) the feature recomputes the term from the positions the role needs and forms the slot's own share of it,
// each component is converted on its own with llrint(c * 2^32), and the integers are summed in list order; then one plain 64-bit
// load, add and store on each of the slot's three plane entries.  A slot has one lane in the whole launch, no lane reads an entry
// another lane writes, and positions are only read: the result is a function of the inputs alone.  No atomic, no inline assembly,
// no LDS on the force path.  llrint of a non-finite share is whatever the conversion instruction gives.
//
// The rule these helpers live by is tgnh_slot_device.h's: a kernel that existed before them compiles to what it compiled to before
// (tools/kernel_isa.py), or does not take the helper.  A new force has no such past and takes all of it.  Who takes what:
//   exception_body (tgnh_nonbonded.hip), exclusion_body (tgnh_ewald.hip) all of it
//   bonded_body, drude_force_body       Fixed3, neg, add_to_planes; the loop is written out there.  for_each_receiver gives
//                                       bonded_forces_kernel, drude_force_kernel and drude_force_energy_kernel the same instructions
//                                       under the same descriptor in another order (lambda or functor; table, sum and entry by value or
//                                       by reference: always the same one), and timing cannot tell that order from the old one: in one
//                                       job launches of identical code differ by as much (profiles/bonded_forces.md)
//   spread_site_forces_kernel           Fixed3 and add_to_planes under its own one-lane-per-row guard (no stride: vs_grid), with
//                                       `Fixed3 sum = {0, 0, 0}`: the default-initialised `Fixed3 sum;` reorders it
//   pair_wave (tgnh_nonbonded.hip)      add_to_planes alone: Fixed3 as its accumulators reorders nb_pair_kernel
#ifndef TGNH_RECEIVER_DEVICE_H_
#define TGNH_RECEIVER_DEVICE_H_
#include "tgnh_receivers.h"
#include "tgnh_position_device.h"

namespace tgnh {

#pragma clang fp contract(off)

// a slot's share of the force in the force buffer's fixed point, x 2^32
struct Fixed3 {
    long long x = 0, y = 0, z = 0;
    __device__ __forceinline__ void add(const Vec3 c) { x += llrint(c.x * 4294967296.0); y += llrint(c.y * 4294967296.0); z += llrint(c.z * 4294967296.0); }
};
__device__ __forceinline__ Vec3 neg(const Vec3 a) { return {-a.x, -a.y, -a.z}; }

// force: [3 * padded] planes x | y | z.  Plain loads and stores: the slot is this lane's alone
__device__ __forceinline__ void add_to_planes(long long* force, const int padded, const int slot, const Fixed3& sum) {
    long long* fx = force + slot;
    long long* fy = force + (size_t)padded + slot;
    long long* fz = force + 2 * (size_t)padded + slot;
    *fx = *fx + sum.x; *fy = *fy + sum.y; *fz = *fz + sum.z;
}

// entry(slot, term, role, Fixed3& sum): adds the slot's share of `term` to sum (and whatever else the feature keeps, by capture)
template <typename Entry>
__device__ __forceinline__ void for_each_receiver(const ReceiverTable& t, long long* force, const int padded, Entry entry) {
    for (long long it = (long long)blockIdx.x * BLOCK + threadIdx.x; it < t.n; it += (long long)gridDim.x * BLOCK) {
        const int r = (int)it;
        const int slot = t.slot[r];
        const int e1 = t.start[r + 1];
        Fixed3 sum;
        for (int e = t.start[r]; e < e1; e++) {
            const int term = t.term[e], role = t.role[e];
            entry(slot, term, role, sum);
        }
        add_to_planes(force, padded, slot, sum);
    }
}

}  // namespace tgnh
#endif
