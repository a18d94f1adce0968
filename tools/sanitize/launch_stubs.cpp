// Host-only sanitizer build: the kernel launchers of the .hip units replaced by stubs that
// fail, so that the host units (csrc/tgnh_*.cpp: topology, tiles, dof, orchestration) can be compiled with g++ -fsanitize and
// exercised through host-only handles (device -1) on a machine without a GPU.  Nothing here ships.
#include "../../openmm_drudenose_amd/csrc/tgnh_internal.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_scale_positions.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_wrap.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_minimize.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_vplanes.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_constraints.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_virtual_sites.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_drude_force.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_bonded.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_nonbonded.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_ewald.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_pme.h"

namespace tgnh {
hipError_t launch_tile(int, int, int, const TileArgs&, int, size_t, hipStream_t) { return hipErrorNoDevice; }
int tile_blocks_per_cu(int, int, int, size_t, bool) { return 2; }
hipError_t launch_step(int, int, int, const TileArgs&, int, size_t, hipStream_t) { return hipErrorNoDevice; }
int step_blocks_per_cu(int, int, int, size_t) { return 2; }
int step_kind_ops2(int) { return 0; }
hipError_t launch_wstep(int, int, bool, const TileArgs&, int, hipStream_t) { return hipErrorNoDevice; }
int wstep_blocks_per_cu(int, int, bool, bool) { return 2; }
hipError_t launch_wke(int, int, int, const TileArgs&, int, hipStream_t) { return hipErrorNoDevice; }
int wke_blocks_per_cu(int, int, int) { return 5; }
hipError_t launch_chain(const ChainArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_big_com(int, const BigComArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_force(int, const ForceArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_plain_ke(int, const void*, const long long*, int, int, double, double*, hipStream_t) { return hipErrorNoDevice; }
size_t tile_lds_bytes(int, int, bool, bool) { return 0; }
hipError_t launch_velinit(int, void*, const int*, int, double, double, unsigned long long, long long, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_drude_stats(int, const void*, const void*, const int*, int, double, double, DrudeStatsRow*, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_cm_momentum(int, const void*, int, CmRow*, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_cm_shift(int, void*, int, const double*, const double*, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_rescale_put(double*, const double*, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_rescale_factors(const double*, const double*, int, double*, uint32_t*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_velm_to_planes(int, const void*, void*, const int2*, int, const void*, const uint32_t*, const uint32_t*, int, uint32_t*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_planes_to_velm(int, const void*, void*, const int2*, int, const void*, const uint32_t*, const uint32_t*, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_constrain_positions(int, const ConstraintArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_constrain_velocities(int, const ConstraintArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_place_sites(int, const SitePlaceArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_spread_site_forces(int, const SiteSpreadArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_drude_force(int, const DrudeForceArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_drude_energy_sum(const double*, int, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_bonded_forces(int, const BondedArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_bonded_energy_sum(const double*, int, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_nonbonded_cells(int, const NonbondedArgs&, hipStream_t, int) { return hipErrorNoDevice; }
hipError_t launch_nonbonded_pairs(int, const NonbondedArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_nonbonded_exceptions(int, const NbExceptionArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_nonbonded_energy_sum(const double*, int, const double*, int, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_ewald_exclusions(int, const EwaldExclusionArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_ewald_reciprocal(int, const EwaldArgs&, hipStream_t, int) { return hipErrorNoDevice; }
hipError_t launch_ewald_energy_sum(const double*, int, double, const double*, int, const double*, double, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_pme(int, const PmeArgs&, hipStream_t, int) { return hipErrorNoDevice; }
hipError_t launch_scale_positions_spans(int, const ScalePosArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_scale_positions_table(int, const ScalePosArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_wrap_spans(int, const WrapArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_wrap_table(int, const WrapArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_frame_spans(int, const WrapArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_frame_table(int, const WrapArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_frame_plain(int, const WrapArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_min_sums(const MinArgs&, int, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_min_decide(const MinArgs&, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_min_update(int, const MinArgs&, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_gather_com(int, const GatherArgs&, hipStream_t) { return hipErrorNoDevice; }
int gather_ke_grid(const GatherArgs&) { return 1; }
hipError_t launch_gather_ke(int, const GatherArgs&, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_gather_rowsum(const double*, int, int, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_gather_chain(const ChainArgs&, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_gather_update(int, const GatherArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_gather_force(int, const GatherArgs&, const void*, long long*, double, double, hipStream_t) { return hipErrorNoDevice; }
}  // namespace tgnh

extern "C" {
tgnh_status tgnh_harness_set_clusters(tgnh_handle, int, const int32_t*, const double*) { return TGNH_ERR_STATE; }
tgnh_status tgnh_harness_shake_positions(tgnh_handle, double, void*) { return TGNH_ERR_STATE; }
tgnh_status tgnh_harness_shake_velocities(tgnh_handle, double, void*) { return TGNH_ERR_STATE; }
tgnh_status tgnh_harness_set_virtual_sites(tgnh_handle, int, const int32_t*, const double*) { return TGNH_ERR_STATE; }
tgnh_status tgnh_harness_virtual_sites(tgnh_handle, void*) { return TGNH_ERR_STATE; }
tgnh_status tgnh_run_harness_constrained(tgnh_handle, const void*, double, double, double, int, void*) { return TGNH_ERR_STATE; }
}
