// tgnh_context.h -- the handle behind the C ABI: its state by concern, and the owner of its device memory.  Host side only
// (tgnh_*.cpp and the host half of tgnh_harness.hip); the kernels see tgnh_internal.h's launch arguments and nothing of this.
#ifndef TGNH_CONTEXT_H_
#define TGNH_CONTEXT_H_

#include <map>
#include <string>
#include <vector>

#include "tgnh_internal.h"
#include "tgnh_by_index.h"
#include "tgnh_minimize.h"
#include "tgnh_receivers.h"

void tgnh_set_error(const std::string& msg);   // sets what tgnh_last_error() returns (tgnh_lifecycle.cpp)

namespace tgnh {
// Device (or pinned host) memory with one owner: freed when the owner goes, or when it is allocated anew.  Reads as the
// pointer it holds.  The handle's device must be current when a buffer is released (tgnh_destroy sees to it).
template <typename T> class DeviceBuf {
    T* p_ = nullptr;
    bool pinned_ = false;
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), pinned_(o.pinned_) { o.p_ = nullptr; }      // (move-only: no copies)
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {           // what it held is released: a table built aside replaces the one in force
        if (this != &o) { reset(); p_ = o.p_; pinned_ = o.pinned_; o.p_ = nullptr; }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    void reset() { if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; }
    // n elements; ext_flags != 0: hipExtMallocWithFlags (TGNH_MEETING_MEM, hipDeviceMallocUncached)
    hipError_t alloc(size_t n, bool zero = false, unsigned ext_flags = 0) {
        reset(); pinned_ = false;
        void* p = nullptr;
        hipError_t e = ext_flags ? hipExtMallocWithFlags(&p, sizeof(T) * n, ext_flags) : hipMalloc(&p, sizeof(T) * n);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        return zero ? hipMemset(p_, 0, sizeof(T) * n) : hipSuccess;
    }
    hipError_t alloc_pinned(size_t n) { reset(); pinned_ = true; return hipHostMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * n, hipHostMallocDefault); }
    hipError_t upload(const T* src, size_t n) {              // a table from the host (an empty one still gets an address)
        hipError_t e = alloc(n ? n : 1);
        return e != hipSuccess || !n ? e : hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};
typedef DeviceBuf<unsigned char> DeviceBytes;   // what the kernels read as real4 / mixed4 of the handle's precision

// The rows of a pass by global index (tgnh_by_index.h): allocated once, at the first call that launches or at the setter that announces launches to come
template <typename Row> struct __attribute__((visibility("hidden"))) RowScratch {
    DeviceBuf<Row> d_rows;            // [rows_allocated]: a row per work-group of the pass, then the result
    int rows_allocated = 0;
    Row h_row{};                      // where the result lands on the host
    // the rows of a pass of `grid` work-groups (zero: cleared when they are allocated); too_small: what to say when grid exceeds them
    tgnh_status ensure(int grid, bool zero, const char* too_small);      // (tgnh_host.h)
};

// A table of receiving slots on the device (tgnh_receivers.h): uploaded at set time, never inside a capture
struct Receivers {
    int n = 0;                        // slots that receive a share of some term
    DeviceBuf<int> d_slot, d_start, d_term;   // [n], [n + 1], [entries]: the inverse in CSR form
    DeviceBuf<unsigned char> d_role;          // [entries]
    hipError_t upload(const ReceiverLists& l) {
        hipError_t e = d_slot.upload(l.slot);
        if (e == hipSuccess) e = d_start.upload(l.start);
        if (e == hipSuccess) e = d_term.upload(l.term);
        if (e == hipSuccess) e = d_role.upload(l.role);
        if (e == hipSuccess) n = (int)l.slot.size();
        return e;
    }
    ReceiverTable view() const { return {d_slot, d_start, d_term, d_role, n}; }
};
}  // namespace tgnh

// Every DeviceBuf below is the handle's own.  Raw pointers are somebody else's memory: the caller's bound arrays (Bound), the
// peers' mailboxes opened over IPC (Exchange::opened, closed -- not freed -- here), a caller's ncclComm_t, and the pointers
// inside an XchgArgs, which point into buffers owned here.
struct tgnh_context {
    tgnh_desc d;                      // scalars only; pointers are nulled after create
    int device = 0;
    bool host_only = false;           // device == -1: topology / dof only, no launches
    struct Topology {                 // host topology (A1), kept for parity queries, and its device tables
        std::vector<double> mass;
        std::vector<int> pair_drude, pair_parent, group, resid, normal;
        std::vector<int> res_count, res_first;
        std::vector<int> tile_start, tile_res;
        std::vector<int2> res_entries;    // per-tile molecule entries
        std::vector<int> big_first, big_count;   // molecules longer than a tile (COM from big_com_kernel)
        int num_big = 0, num_tiles = 0;
        std::vector<uint32_t> meta;
        std::vector<int2> wave_tile;      // wave tiles (empty: some molecule or pair does not fit a wavefront)
        std::vector<uint32_t> wmeta;
        std::vector<uint32_t> tile_pat, wtile_pat;    // per 512-slot tile: period | molecules << 8 | pattern << 16; per wave tile: period | pattern << 8; 0 = none
        std::vector<uint32_t> pattern, wpattern;      // 64 words per pattern
        std::vector<double> wpat_mass;                // beside wpattern: the descriptor masses of a wave pattern's slots, 64 per pattern
        bool wpat_all_uniform = false;                // every wave tile is patterned, and every slot's mass is its pattern entry's
        // wpat_all_uniform: where the velocity planes keep a MASSIVE slot (a massless one has no word there) -- word
        // wtile_base[tile] + wpat_off[pattern * 64 + lane] of each plane.  wtile_base: [num_wtiles + 1], every entry a multiple of
        // 16 words (a 128-byte line of 8-byte words), the last one the planes' stride; wpat_off: beside wpattern, per LANE (not per
        // place in the period), the massive slots of the tile before that lane.  Empty otherwise.
        std::vector<uint32_t> wtile_base, wpat_off;
        int num_wtiles = 0;
        tgnh::DeviceBuf<uint32_t> d_meta, d_wmeta, d_tile_pat, d_pattern, d_wpattern;
        tgnh::DeviceBuf<int> d_tile_start, d_tile_res;
        tgnh::DeviceBuf<int2> d_res_table, d_wave_tile, d_big_table;
        tgnh::DeviceBytes d_big_com;
    } topo;
    // the gather path: taken when the tiles cannot hold the topology (reason says why); the reference's index lists, per particle
    struct Gather {
        bool generic = false;
        bool chain = false;               // ... and its chain too: more than 34 thermostats, or links that do not fit the LDS (gather_chain_kernel)
        std::string reason;
        std::vector<int2> res_table;
        std::vector<int> resid, partner;
        int com_lanes = 64;
        tgnh::DeviceBuf<int> d_group, d_resid, d_partner;
        tgnh::DeviceBuf<int2> d_res_table;
        tgnh::DeviceBytes d_com;
        tgnh::DeviceBuf<double> d_scratch;    // chains longer than 4 links of more than 34 thermostats: a row of 4 C + 1 doubles each
    } gather;
    struct ByIndex {                  // the passes by global index on a tiled handle (the velocity draw, the Drude statistics): the gather
        tgnh::DeviceBuf<int> d_partner;   // path's partner table, built by whichever of them is called first (device_partner_table)
    } by_index;
    tgnh::RowScratch<tgnh::DrudeStatsRow> dstats;      // tgnh_get_drude_statistics
    struct CmMotion : tgnh::RowScratch<tgnh::CmRow> {  // tgnh_get_momentum / tgnh_remove_cm_motion, tgnh_set_cm_motion_removal (tgnh_velocities.cpp)
        int every = 0;                    // tgnh_set_cm_motion_removal: remove before every step whose number is a multiple of this (0: never)
    } cmm;
    struct Rescale {                  // tgnh_scale_velocities / tgnh_rescale_to_temperature: allocated at the first call that launches
        tgnh::DeviceBuf<double> d_buf;    // (or at tgnh_set_velocity_rescaling: never inside somebody's stream capture) [2 NT]: the factors
                                          // the rescale launch reads -- never the thermostat block's scale entries --, then the targets N kT
        bool applied = false;             // a call has written the factors (tgnh_get_rescale_factors answers)
        int every = 0;                    // tgnh_set_velocity_rescaling: rescale before every step whose number is a multiple of this (0: never)
        double temperature = 0, drude_temperature = 0;   // ... to these
    } resc;
    struct Molecules {                // what tgnh_scale_positions moves rigidly (tgnh_positions.cpp): the caller's labels, or the descriptor's resid
        struct Table {                    // host side, built as a whole from one set of labels
            std::vector<int> mol_of;          // [N] labels renumbered 0..count-1 in order of first appearance
            int count = 0;
            std::vector<int> mem_start, members;   // [count + 1], [N]: the slots by molecule, ascending within one
            bool spans = false;               // every molecule a run of consecutive slots no longer than a wavefront: the span kernel serves it
            std::vector<int> span_first;      // [spans + 1] spans of whole molecules, <= 64 slots each
            std::vector<unsigned long long> span_heads;   // [spans] bit l: a molecule starts at lane l of the span
            std::vector<int> span_out;        // [spans] tgnh_write_frame without Drude slots: the output index of the span's first kept slot
            std::vector<unsigned long long> span_drude;   // [spans] ... and bit l: lane l of the span is a Drude slot
        } t;
        bool set = false;                 // t is in force (tgnh_set_molecules, or the default resolved at the first call that needed one)
        bool on_device = false;           // the copies below are t's: made at tgnh_set_molecules on a device handle or at the first launching call
        tgnh::DeviceBuf<int> d_span_first, d_mol_of, d_mem_start, d_members;      // spans: the first; otherwise the other three
        tgnh::DeviceBuf<unsigned long long> d_span_heads;
        tgnh::DeviceBuf<int> d_span_out;  // spans: the two words more of a frame without Drude slots
        tgnh::DeviceBuf<unsigned long long> d_span_drude;
        tgnh::DeviceBuf<double> d_shift;  // [3 count] table path: d of every molecule, written by its first launch
        void drop_device() { on_device = false; d_span_first.reset(); d_mol_of.reset(); d_mem_start.reset(); d_members.reset(); d_span_heads.reset(); d_shift.reset(); d_span_out.reset(); d_span_drude.reset(); }
    } mol;
    struct PeriodicBox {              // tgnh_set_periodic_box (tgnh_frames.cpp): host side only, handed to every launch by value
        bool set = false;
        double a[3] = {0, 0, 0}, b[3] = {0, 0, 0}, c[3] = {0, 0, 0};     // the caller's doubles, bit for bit
    } box;
    struct Frames {                   // tgnh_write_frame without Drude slots, by slot index (the table form, the plain frame): no molecule table in it
        std::vector<int> out_index;       // [N] output index of a slot, -1 for a Drude slot; built at the first call that asks (frame_index)
        int kept = -1;                    // N minus the Drude slots (-1: not counted yet)
        tgnh::DeviceBuf<int> d_out_index; // made once, never inside a capture
    } frames;
    struct PositionSnapshot {         // tgnh_scale_positions(save) -> tgnh_restore_positions: allocated at the first saving call
        tgnh::DeviceBytes d_posq, d_corr; // one copy of posq, and of posq_correction in mixed precision
        bool taken = false;               // a saving call has filled it
        bool valid = false;               // ... and tgnh_bind_buffers has not rebound a position array since
        const void *of_posq = nullptr, *of_corr = nullptr;     // the arrays it was read from
    } snap;
    struct Minimize {                 // tgnh_minimize_begin .. tgnh_minimize_end (tgnh_minimize.cpp): everything is allocated at begin, never inside a capture
        bool active = false;              // between a begin that succeeded and the next end
        double* work = nullptr;           // the caller's [3 N] doubles: the minimiser's velocity
        int64_t moving = 0;               // this handle's moving slots
        tgnh::DeviceBuf<unsigned char> d_mask;     // [N] non-zero: the slot moves
        tgnh::DeviceBuf<double> d_rows;   // [index_grid(N) + 1][4]: a row per work-group of the sums pass, then the four sums an all-reduce adds in place
        tgnh::DeviceBuf<tgnh::MinState> d_state;
        tgnh::MinState h_state{};         // what begin uploads, and where tgnh_get_minimize_state's copy lands
        void drop() { active = false; work = nullptr; moving = 0; d_mask.reset(); d_rows.reset(); d_state.reset(); }
    } minim;
    struct Constraints {              // tgnh_set_constraint_clusters (tgnh_constraints.cpp): the direct solver's cluster table, rows sorted by smallest slot
        int count = 0;                    // clusters in force (a host-only handle keeps the count and nothing else)
        tgnh::DeviceBuf<int4> d_atoms;    // [count] uploaded at set time, never inside a capture
        tgnh::DeviceBuf<double4> d_invmass;   // [count] from the descriptor's masses
        tgnh::DeviceBuf<double> d_d2;     // [3][count]
        tgnh::DeviceBuf<uint32_t> d_pairs;    // [count]
        void drop() { count = 0; d_atoms.reset(); d_invmass.reset(); d_d2.reset(); d_pairs.reset(); }
    } cons;
    // The four tables of the library's forces below are built aside by their setters and moved in whole; a clear assigns a fresh value.
    struct VirtualSites {             // tgnh_set_virtual_sites (tgnh_virtual_sites.cpp): the site table, rows sorted by site slot, and its inverse
        int count = 0;                    // sites in force (a host-only handle keeps the count and nothing else)
        tgnh::DeviceBuf<int4> d_atoms;    // [count] (site, p1, p2, p3), uploaded at set time, never inside a capture
        tgnh::DeviceBuf<int> d_kind;      // [count]
        tgnh::DeviceBuf<double> d_params; // [12][count]
        tgnh::Receivers recv;             // the slots that receive a share of some site's force
    } vsites;
    struct DrudeForce {               // tgnh_set_drude_force (tgnh_drude_force.cpp): the rows in the descriptor's pair order, the screened pairs, the inverse
        int rows = 0, screened = 0;       // terms in force (a host-only handle keeps the counts and nothing else)
        bool energy_launched = false;     // a want_energy launch has filled d_energy's rows since the table was set
        tgnh::DeviceBuf<int4> d_atoms;    // [rows] (p, p1, p2, p3), uploaded at set time, never inside a capture
        tgnh::DeviceBuf<int> d_p4;        // [rows]
        tgnh::DeviceBuf<double> d_k;      // [3][rows] k1, k2, k3
        tgnh::DeviceBuf<int2> d_pair_rows;        // [screened]
        tgnh::DeviceBuf<double2> d_pair_par;      // [screened] (a, K)
        tgnh::Receivers recv;             // the slots that receive a share of some term
        tgnh::DeviceBuf<double> d_energy; // [index_grid(recv.n) + 1][4]: a row per work-group of the launch, then the totals; allocated at set time
    } dforce;
    struct BondedForces {             // tgnh_set_bonded_forces (tgnh_bonded.cpp): the three tables in the caller's order and their one inverse
        int bonds = 0, angles = 0, torsions = 0;  // terms in force (a host-only handle keeps the counts and nothing else)
        bool energy_launched = false;     // a want_energy launch has filled d_energy's rows since the tables were set
        tgnh::DeviceBuf<int2> d_bond_atoms;       // [bonds] (p1, p2), uploaded at set time, never inside a capture
        tgnh::DeviceBuf<double2> d_bond_par;      // [bonds] (length, k)
        tgnh::DeviceBuf<int4> d_angle_atoms;      // [angles] (p1, p2, p3, 0)
        tgnh::DeviceBuf<double2> d_angle_par;     // [angles] (angle, k)
        tgnh::DeviceBuf<int4> d_torsion_atoms;    // [torsions]
        tgnh::DeviceBuf<int> d_torsion_n;         // [torsions]
        tgnh::DeviceBuf<double> d_torsion_par;    // [3][torsions] cos(phase), sin(phase), k
        tgnh::Receivers recv;             // the slots that receive a share of some term
        tgnh::DeviceBuf<double> d_energy; // [index_grid(recv.n) + 1][4]: a row per work-group of the launch, then the totals; allocated at set time
        bool empty() const { return bonds + angles + torsions == 0; }
    } bonded;
    struct Nonbonded {                // tgnh_set_nonbonded_force (tgnh_nonbonded.cpp): the particle table, the exclusion lists, the evaluated exceptions' inverse
        int particles = 0, exceptions = 0, evaluated = 0;   // in force (a host-only handle keeps these, the scalars below, and nothing else)
        double cutoff = 0, dielectric = 0, krf = 0, crf = 0;
        bool energy_launched = false;     // a want_energy call has filled the rows since the tables were set
        int energy_rows = 0;              // ... and the pair launch of the last such call wrote this many
        int cells_allocated = 0;          // what the per-cell buffers below hold; they grow at the first call that needs more, never inside a capture
        tgnh::DeviceBuf<double> d_par;            // [particles][3] charge, sigma, epsilon; uploaded at set time, as everything down to d_totals
        tgnh::DeviceBuf<int> d_excl_start, d_excl;        // [particles + 1], [2 exceptions]: a slot's excluded partners, ascending
        tgnh::DeviceBuf<int2> d_excl_range;       // [particles] (lowest, highest) excluded partner, (1, 0): none
        tgnh::DeviceBuf<int2> d_exc_atoms;        // [evaluated] (p1, p2)
        tgnh::DeviceBuf<double> d_exc_par;        // [evaluated][3] chargeProd, sigma, epsilon
        tgnh::Receivers recv;                     // the slots that receive a share of some evaluated exception
        tgnh::DeviceBuf<double> d_exc_rows;       // [index_grid(recv.n)][4]
        tgnh::DeviceBuf<int> d_cell_of, d_placed, d_sorted_slot, d_n_chunks;   // [particles] x 3, [1]: the cell build's per-slot scratch
        tgnh::DeviceBuf<double> d_sorted;         // [6][particles]
        tgnh::DeviceBuf<int2> d_sorted_range;     // [particles]
        tgnh::DeviceBuf<double> d_totals;         // [4] where the energy's sum lands
        tgnh::DeviceBuf<int> d_count, d_cell_start;       // [2 cells_allocated], [cells_allocated + 1]
        tgnh::DeviceBuf<int2> d_chunks;           // [cells_allocated + ceil(particles / 64)]
        tgnh::DeviceBuf<double> d_pair_rows;      // [pair grid of cells_allocated][4]
        std::vector<double> h_charge;             // [particles] the table's charges, and
        std::vector<int2> h_exc;                  // [exceptions] every row's (p1, p2) in the caller's order: what tgnh_set_nonbonded_ewald builds from (a handle with a device only)
        hipStream_t last_stream = nullptr;        // of the last tgnh_compute_nonbonded_force: a setter has no stream of its own to ask about a capture
    } nonbonded;
    struct Ewald {                    // tgnh_set_nonbonded_ewald (tgnh_ewald.cpp), on top of the table above; tgnh_set_nonbonded_force assigns a fresh value
        bool on = false;
        int kmax[3] = {0, 0, 0};
        double alpha = 0, tsp = 0, a4 = 0;        // tsp = 2 alpha / sqrt(pi), a4 = 4 (alpha alpha)
        double e_self = 0, bg_num = 0;            // -K (alpha / sqrt(pi)) sum q^2 in slot order; ((pi K) (Q Q)) / (2 (alpha alpha))
        int vectors = 0, parts = 0;               // M; ceil(particles / EW_PART)   (a host-only handle keeps the scalars down to here and nothing else)
        int corrected = 0;                        // exception rows whose particles' charges have a non-zero product
        bool energy_launched = false;             // a want_energy call has filled the rows since Ewald was set
        tgnh::DeviceBuf<int4> d_kvec;             // [vectors] (nx, ny, nz, 0); uploaded at set time, as everything below is allocated there
        tgnh::DeviceBuf<double2> d_part_rows;     // [parts][vectors]
        tgnh::DeviceBuf<double> d_coef;           // [vectors][5]
        tgnh::DeviceBuf<double> d_rec_rows;       // [index_grid(vectors)][4]
        tgnh::DeviceBuf<int2> d_exc_atoms;        // [corrected] (p1, p2)
        tgnh::Receivers recv;                     // the slots that receive a share of some corrected row
        tgnh::DeviceBuf<double> d_exc_rows;       // [index_grid(recv.n)][4]
        tgnh::DeviceBuf<double> d_misc;           // [2] {E_bg, (4 (pi K)) / V} of the last want_energy call's box
        tgnh::DeviceBuf<double> d_totals;         // [4] where the energy's sum lands
        // the other form of the setting: tgnh_set_nonbonded_pme (tgnh_pme.cpp).  `on` with pme: the mesh forms the reciprocal part, vectors == 0
        bool pme = false;
        int grid[3] = {0, 0, 0};                  // nx, ny, nz   (a host-only handle keeps these two lines and nothing below)
        double pi2 = 0, alpha2 = 0;               // pi pi, alpha alpha
        bool grids_filled = false;                // an eager tgnh_compute_nonbonded_force has run since PME was set
        tgnh::DeviceBuf<long long> d_charge;      // [nz][ny][nx] the spread charges x 2^48
        tgnh::DeviceBuf<double2> d_work;          // [nz][ny][nx] the transforms' complex grid
        tgnh::DeviceBuf<double> d_potential;      // [nz][ny][nx] phi
        tgnh::DeviceBuf<double2> d_twiddle[3];    // [N_d] w^k
        tgnh::DeviceBuf<double> d_modulus[3];     // [N_d] |b_d(m)|^2      (d_rec_rows: [pme_fft_grid(grid, 2)][4])
    } ewald;
    struct Thermostat {               // dof bookkeeping (A2) and the thermostat block
        std::vector<double> h_state;      // host copy of the initial thermostat block
        std::vector<double> local_terms, global_terms;   // per thermostat, before CMM correction
        std::vector<double> dof, nkbt;
        double realkbT = 0, drudekbT = 0;
        tgnh::ChainLayout L{};
        tgnh::DeviceBuf<double> d_partials;
        tgnh::DeviceBuf<double> d_state;      // thermostat block
        tgnh::DeviceBuf<double> d_stage;      // same layout: where an in-kernel chain leaves the advanced block
        tgnh::DeviceBuf<double> d_scalar;     // plain KE: [0] the result, [1 ..] work-group partials
    } thermo;
    struct LaunchConfig {             // fixed at create (the grids: filled in at the first launch of their kind)
        int grid = 0, gb = 1;
        int num_cus = 256, grid_override = 0;
        std::map<int, int> grid_cache;    // ops (+hard-wall bit) -> persistent grid size
        bool alternate_sweeps = true;
        int inline_sum_rows = tgnh::CHAIN_INLINE_SUM_ROWS;
        bool inline_sum_all = false;      // more rows than that (and < 2 M slots): all four wavefronts of the rescale launch sum them (sum_rows = 2)
        bool carry_ok = false;            // TGNH_FLAG_TRUST_STATE_CHANGED is in effect for this handle (set, unsharded, no molecule spans two groups)
        bool inline_chain = false;        // numNHChains == 1: the chain runs inside the rescale launch
        bool wave_ke = false;             // the KE passes run over the wave tiles (wke_kernel)
        int resident_grid[5][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};   // step_kernel's grid by kind and hard wall
        int resident_share = 1;
        int wresident_per_cu = 0, wresident_grid = 0;   // the same for wstep_kernel (0: none, or no wave tiles)
        int resident_per_cu = 0;          // work-groups of step_kernel per compute unit that the census at create found resident together (0: none -- the handle steps the DEFER_SCALE way)
    } cfg;
    // The one-launch step's velocities as three planes (tgnh_vplanes.hip): the library's own copy of velm's x, y, z
    // between flushes of a DEFER_SCALE | RESIDENT_STEP sequence.  Owed::planes_live says which of the two holds the velocities.
    struct VelPlanes {
        tgnh::DeviceBytes d_planes;       // x | y | z of Prec::mixed, the massive slots only, stride `stride`: allocated at create where the handle can take them, never later
        tgnh::DeviceBytes d_invm;         // [patterns][64] Prec::mixed: 1 / Topology::wpat_mass (0 for a massless slot), what velm's w must hold
        tgnh::DeviceBuf<uint32_t> d_base, d_off;    // Topology::wtile_base, wpat_off
        int stride = 0;                   // words of a plane: wtile_base's last entry
        tgnh::DeviceBuf<uint32_t> d_mismatch;   // the first conversion of a bind ORs 1 in here when some slot's w is not its table entry
        int verdict = 0;                  // of that check: 0 not made yet, 1 the table is velm's w, -1 it is not (the handle stays on velm)
        int streak = 0;                   // one-launch steps in a row since the last settle (enter_planes' hysteresis)
        bool pinned = false;              // steps were recorded into a graph while velm held the velocities: the handle stays there
        hipStream_t stream = nullptr;     // of the launch that last wrote the planes (tgnh_state_changed has no stream of its own)
        bool usable() const { return d_planes.get() != nullptr && verdict >= 0 && !pinned; }
    } vp;
    // What a step still owes: work an entry point has left to a later launch, and what the last launches left behind.
    struct Owed {
        // the first eight are bits 0..7 of tgnh_get_pending_state, in this order; the last five are not reported
        bool end_pending = false;         // RESIDENT_STEP: the whole end half of the last step waits for the next step_begin's launch
        bool scale_pending = false;       // DEFER_SCALE: velm lags by scale[]
        bool kick_pending = false;        // DEFER_SCALE: velm also lags by the second half kick (force buffer unchanged since)
        bool first_half_done = false;     // DEFER_SCALE: chain for the coming step's first half already run
        bool chain_pending = false;       // summed KE waits for the next rescale launch to run the chain
        bool sum_pending = false;         // with chain_pending: the partial rows are not summed yet either (the rescale launch does both)
        bool xwait_pending = false;       // with chain_pending: the sums were sent over the mailboxes, nobody has waited for the peers' yet
        bool stage_pending = false;       // d_stage is newer than d_state; the next chain_kernel launch commits it
        bool ke_carry = false;            // (bit 9) TRUST_STATE_CHANGED: ke_post of the last end half IS the kinetic energy of the stored velocities
        bool planes_live = false;         // (bit 10) the velocities live in VelPlanes::d_planes; velm's x, y, z are as old as the last settle (settle_end leaves)
        bool chain_pending_twice = false; // with chain_pending: both chain halves (DEFER_SCALE)
        bool carry_pending = false;       // ... and that KE is the last chain's ke_post (ChainArgs::ke_carry), not ke_red
        bool tail_summed = false;         // the last KE launch summed its rows itself (wke_kernel's tail sum): no row-sum launch
        bool end_folded = false;          // the last fused end half left the kick to its rescale launch (OP_PREKICK: algorithmic bytes of KID_SCALE)
        bool g_com_fresh = false;         // gather path: the COM table is of the velocities as they are (set by a KE pass; cleared by the next launch that writes velocities and on entry to every entry point)
        enum : uint32_t { BIT_SWEEP_REVERSE = 1u << 8 };      // (Run::sweep_reverse, reported beside these)
        uint32_t bits() const {           // the layout include/drude_tgnh.h documents, written down here and nowhere else
            return end_pending | scale_pending << 1 | kick_pending << 2 | first_half_done << 3 | chain_pending << 4 | sum_pending << 5 |
                   xwait_pending << 6 | stage_pending << 7 | ke_carry << 9 | planes_live << 10;
        }
        void chain_owed(bool twice) { chain_pending = true; chain_pending_twice = twice; }           // (whoever leaves it says what else the rescale launch does: sum_pending, xwait_pending, carry_pending)
        void chain_ran() { chain_pending = sum_pending = xwait_pending = carry_pending = false; }     // (whoever ran it says where the block now lies: stage_pending)
        void velocities_current() { scale_pending = kick_pending = false; }
        void end_half_deferred(bool kick) { scale_pending = first_half_done = true; kick_pending = kick; }   // DEFER_SCALE: both chain halves are in scale[], velm lags
        void resident_settled() { end_pending = first_half_done = false; velocities_current(); chain_pending = sum_pending = xwait_pending = false; }
        void thermostat_reset() { end_pending = first_half_done = false; velocities_current(); chain_pending = stage_pending = carry_pending = ke_carry = false; }
    } owed;
    struct Run {
        double time = 0;
        int64_t step_count = 0;
        int sweep_reverse = 0;            // direction of the next streaming launch (alternates)
        int ke_parts = 0;                 // rows of partial sums the last KE launch wrote
    } run;
    struct Bound {                    // the caller's arrays (tgnh_bind_buffers)
        void *posq = nullptr, *posq_corr = nullptr, *velm = nullptr, *pos_delta = nullptr;
        const void* force = nullptr;
    } bound;
    struct Status {
        tgnh::DeviceBuf<uint32_t> d_word;
        tgnh::DeviceBuf<uint32_t> h_seen;    // pinned: where read-backs of the status word land (periodic, and at every query)
        int failed_code = 0;                 // sticky: a failure the device reported (note_status); every later entry returns it
        std::string failed;
    } status;
    struct Meeting {                  // where the work-groups of one launch meet (step_kernel, wstep_kernel, wke_kernel's tail sum)
        tgnh::DeviceBuf<unsigned int> d_sync;           // launch number
        tgnh::DeviceBuf<unsigned long long> d_rows;     // ... and the tagged rows (uncached)
        tgnh::DeviceBuf<unsigned long long> self_box;      // RESIDENT_STEP without a sharded exchange: a private one-rank mailbox
        tgnh::DeviceBuf<unsigned long long> d_self_misc;   // ... its counter, latch and peer table
        tgnh::XchgArgs self_x{};
    } meet;
    struct Exchange {                 // the kinetic-energy sums across ranks: a hook, RCCL, or the mailboxes (which replace the hook when attached)
        tgnh_allreduce_fn allreduce = nullptr;
        void* allreduce_user = nullptr;
        void* rccl_comm = nullptr;        // ncclComm_t: the library enqueues ncclAllReduce itself (tgnh_rccl_init / tgnh_set_rccl_comm)
        bool rccl_owned = false;
        tgnh::XchgArgs args{};
        bool on = false;
        int world = 0, rank = 0;
        tgnh::DeviceBuf<unsigned long long> mailbox;     // mine (uncached device memory)
        tgnh::DeviceBuf<unsigned long long*> d_peers;    // device table of every rank's mailbox
        std::vector<void*> opened;                       // peers' mailboxes opened by IPC (to close)
        tgnh::DeviceBuf<unsigned long long> d_seq;
        tgnh::DeviceBuf<unsigned int> d_dead;
        tgnh::DeviceBuf<unsigned long long> d_stat;      // mailbox wait statistics (XchgArgs::stat)
        void close_peers() { for (void* p : opened) (void)hipIpcCloseMemHandle(p); opened.clear(); }
        ~Exchange() { close_peers(); }
    } xchg;
    struct Harness {                  // the test harness's call-outs (tgnh_harness.hip, tgnh_harness_host.cpp)
        tgnh::DeviceBuf<int4> d_cl_atoms, d_vs_atoms;
        tgnh::DeviceBuf<double> d_cl_dist, d_vs_w;
        int num_clusters = 0, num_sites = 0;
        tgnh::DeviceBuf<uint8_t> d_sflag;         // packed tether sites (ForceArgs::sflag / sbase / sites), tgnh_harness_pack_sites
        tgnh::DeviceBuf<uint32_t> d_sbase;
        tgnh::DeviceBytes d_sites;
        int lat_k = 0, lat_side = 0, lat_mol0 = 0;              // ... or lattice sites: the hint (lat_k = 0: none), and whether pack_sites found it to hold
        double lat_spacing = 0;
        std::vector<double> lat_geom;
        bool lat_on = false;
        tgnh::DeviceBuf<unsigned char> d_lat_tab;
        tgnh::DeviceBytes d_g_x0;         // gather path: the tether sites as tgnh_harness_pack_sites was handed them
    } harness;
    struct Timing {
        bool on = false;
        int only = -1;                    // >= 0: only this kernel id is timed
        struct Ev { hipEvent_t a, b; int kid; };
        std::vector<Ev> ev_pool;
        size_t ev_used = 0;
        double t_total[tgnh::KID_COUNT] = {0};
        int64_t t_count[tgnh::KID_COUNT] = {0};
        ~Timing() { for (auto& e : ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); } }
    } timing;
};

#endif
