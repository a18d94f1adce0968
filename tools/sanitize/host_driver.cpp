// Stand-alone driver of the host-only sanitizer build (run_host_driver_asan.sh): the host side of tgnh_set_temperatures and
// tgnh_set_velocities_to_temperature, the argument checks of the centre-of-mass and velocity-rescaling calls, the molecule table of tgnh_scale_positions, and the periodic
// box, tgnh_get_frame_count and the argument order of tgnh_wrap_molecules / tgnh_write_frame, and the minimiser's argument checks and refusals, through a host-only handle (device -1),
// no Python in the process.  What needs a device --
// the upload of the retargeted block, the partner table's first use and the launch -- is not reached here.  And, without a handle, the
// inversion of a force's shares into receiving slots (tgnh_receivers.h) against a brute-force restatement.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/drude_tgnh.h"
#include "../../openmm_drudenose_amd/csrc/tgnh_receivers.h"

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "host_driver: %s failed (line %d): %s\n", #cond, __LINE__, tgnh_last_error()); return 1; } } while (0)

static int run(int mode, int chains, int drude_chains) {
    const int mols = 37, N = 5 * mols;                          // SWM4 water: O, D, H1, H2, M (massless)
    std::vector<double> mass;
    std::vector<int32_t> pd, pp, group(N, 0), resid;
    for (int m = 0; m < mols; m++) {
        const double mm[5] = {15.6, 0.4, 1.0, 1.0, 0.0};
        for (int k = 0; k < 5; k++) { mass.push_back(mm[k]); resid.push_back(m); }
        pd.push_back(5 * m + 1); pp.push_back(5 * m);
    }
    tgnh_desc d{};
    d.struct_size = sizeof(d); d.mode = mode; d.precision = TGNH_PREC_MIXED; d.device = -1;
    d.num_particles = N; d.padded_num_particles = (N + 31) / 32 * 32; d.num_pairs = mols; d.num_groups = 1; d.num_residues = mols;
    d.mass = mass.data(); d.pair_drude = pd.data(); d.pair_parent = pp.data(); d.group = group.data(); d.resid = resid.data();
    d.kB = 8.31446261815324e-3; d.temperature = 300; d.coupling_time = 0.1; d.drude_temperature = 1; d.drude_coupling_time = 0.005;
    d.step_size = 0.001; d.drude_steps_per_real_step = 20; d.num_nh_chains = chains; d.use_drude_nh_chains = drude_chains; d.use_com_temp_group = 1;
    tgnh_handle a = nullptr, b = nullptr;
    EXPECT(tgnh_create(&d, &a) == TGNH_OK);
    d.temperature = 350; d.drude_temperature = 2;
    EXPECT(tgnh_create(&d, &b) == TGNH_OK);
    EXPECT(tgnh_set_temperatures(a, NAN, 1, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_temperatures(a, 300, -1, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_temperatures(nullptr, 300, 1, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_temperatures(a, 350, 2, nullptr) == TGNH_OK);
    int nt = 0, len = 0;
    // the velocity planes' layout (tgnh_get_topology 17: stride, number of bases, bases, lane offsets): four wave tiles of 12, 12, 12
    // and 1 molecules with 4 massive slots each, every segment on a 16-word line; one pattern, the massless slot last of five
    EXPECT(tgnh_get_topology_len(a, 17, &len) == TGNH_OK && len == 2 + 5 + 64);
    std::vector<int32_t> lay(len);
    EXPECT(tgnh_get_topology(a, 17, lay.data()) == TGNH_OK && lay[0] == 160 && lay[1] == 5);
    EXPECT(lay[2] == 0 && lay[3] == 48 && lay[4] == 96 && lay[5] == 144 && lay[6] == 160);
    for (int lane = 0; lane < 64; lane++) EXPECT(lay[7 + lane] == lane - lane / 5);
    EXPECT(tgnh_get_num_thermostats(a, &nt) == TGNH_OK && nt >= 3);
    std::vector<double> da(nt), na(nt), db(nt), nb(nt);
    EXPECT(tgnh_get_dof(a, da.data(), na.data()) == TGNH_OK && tgnh_get_dof(b, db.data(), nb.data()) == TGNH_OK);
    for (int i = 0; i < nt; i++) EXPECT(da[i] == db[i] && na[i] == nb[i]);
    for (int which = 0; which < 4; which++) {                    // untouched chains are still the initial ones: all four arrays agree
        EXPECT(tgnh_get_thermostat_len(a, which, &len) == TGNH_OK);
        std::vector<double> xa(len), xb(len);
        EXPECT(tgnh_get_thermostat_state(a, which, nullptr, xa.data()) == TGNH_OK && tgnh_get_thermostat_state(b, which, nullptr, xb.data()) == TGNH_OK);
        if (which == 3) for (int i = 0; i < len; i++) EXPECT(xa[i] == xb[i]);
    }
    EXPECT(tgnh_set_velocities_to_temperature(a, -1, 1, 1, 0, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_velocities_to_temperature(a, 300, INFINITY, 1, 0, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_velocities_to_temperature(a, 300, 1, 1, -1, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_velocities_to_temperature(nullptr, 300, 1, 1, 0, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_velocities_to_temperature(a, 300, 1, ~0ull, 1ll << 40, nullptr) == TGNH_ERR_STATE);      // host-only: nothing launches
    // centre-of-mass motion: the argument checks and the host-only refusals (nothing launches, no scratch is allocated)
    tgnh_momentum mom{};
    const double dv[3] = {0.1, -0.2, 0.3}, odd[3] = {0.0, NAN, 0.0};
    EXPECT(tgnh_get_momentum(a, nullptr, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_get_momentum(a, nullptr, &mom) == TGNH_ERR_ARG);                                               // struct_size 0
    mom.struct_size = sizeof(mom);
    EXPECT(tgnh_get_momentum(nullptr, nullptr, &mom) == TGNH_ERR_ARG);
    EXPECT(tgnh_get_momentum(a, nullptr, &mom) == TGNH_ERR_STATE && mom.massive == 0 && mom.mass == 0);
    EXPECT(tgnh_shift_velocities(a, nullptr, nullptr) == TGNH_ERR_ARG && tgnh_shift_velocities(a, odd, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_shift_velocities(a, dv, nullptr) == TGNH_ERR_STATE && tgnh_remove_cm_motion(a, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_set_cm_motion_removal(a, -1) == TGNH_ERR_ARG && tgnh_set_cm_motion_removal(nullptr, 1) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_cm_motion_removal(a, 5) == TGNH_OK && tgnh_step_begin(a, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_set_cm_motion_removal(a, 0) == TGNH_OK);
    // velocity rescaling: the argument checks, the targets formed on the host for other temperatures, the host-only refusals
    std::vector<double> fac(nt, 1.25), got(nt, 7.0), nkt0(nt), nkt1(nt);
    EXPECT(tgnh_get_dof(a, nullptr, nkt0.data()) == TGNH_OK);
    EXPECT(tgnh_scale_velocities(a, nullptr, nt, nullptr) == TGNH_ERR_ARG && tgnh_scale_velocities(a, fac.data(), nt - 1, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_scale_velocities(nullptr, fac.data(), nt, nullptr) == TGNH_ERR_ARG);
    fac[0] = -0.5;
    EXPECT(tgnh_scale_velocities(a, fac.data(), nt, nullptr) == TGNH_ERR_ARG);
    fac[0] = NAN;
    EXPECT(tgnh_scale_velocities(a, fac.data(), nt, nullptr) == TGNH_ERR_ARG);
    fac[0] = 0.0;
    EXPECT(tgnh_scale_velocities(a, fac.data(), nt, nullptr) == TGNH_ERR_STATE);                               // host-only: nothing launches
    EXPECT(tgnh_rescale_to_temperature(a, NAN, 1, nullptr) == TGNH_ERR_ARG && tgnh_rescale_to_temperature(a, 300, -1, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_rescale_to_temperature(a, 350, 2, nullptr) == TGNH_ERR_STATE && tgnh_rescale_to_temperature(a, 0, 0, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_get_rescale_factors(a, nullptr, nullptr) == TGNH_ERR_ARG && tgnh_get_rescale_factors(a, nullptr, got.data()) == TGNH_ERR_STATE && got[0] == 7.0);
    EXPECT(tgnh_set_velocity_rescaling(a, -1, 300, 1) == TGNH_ERR_ARG && tgnh_set_velocity_rescaling(a, 1, NAN, 1) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_velocity_rescaling(a, 4, 350, 2) == TGNH_OK && tgnh_step_begin(a, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_set_velocity_rescaling(a, 0, 350, 2) == TGNH_OK);
    EXPECT(tgnh_get_dof(a, nullptr, nkt1.data()) == TGNH_OK && nkt0 == nkt1);                                  // the baths are whose they were
    // the molecule table: the default from resid, labels in two runs and longer than a wavefront, a split pair, the host-only refusals
    int nmol = 0;
    std::vector<int32_t> lab(N), out(N, -1);
    EXPECT(tgnh_get_num_molecules(a, &nmol) == TGNH_OK && nmol == mols);
    for (int i = 0; i < N; i++) lab[i] = i < 70 ? -5 : (i / 5 == mols - 1 ? -5 : 1000000 + i / 5);              // 75 slots in two runs, the rest per water
    EXPECT(tgnh_set_molecules(a, lab.data()) == TGNH_OK && tgnh_get_num_molecules(a, &nmol) == TGNH_OK && nmol == mols - 14);
    EXPECT(tgnh_get_molecules(a, out.data()) == TGNH_OK && out[0] == 0 && out[N - 1] == 0 && out[70] == 1 && out[N - 6] == mols - 15);
    lab[1] = 7;                                                                                                // Drude of pair 0 alone
    EXPECT(tgnh_set_molecules(a, lab.data()) == TGNH_ERR_ARG && tgnh_get_num_molecules(a, &nmol) == TGNH_OK && nmol == mols - 14);
    EXPECT(tgnh_set_molecules(a, nullptr) == TGNH_OK && tgnh_get_num_molecules(a, &nmol) == TGNH_OK && nmol == mols);
    const double sc[3] = {1.01, 0.99, 1.0}, bad[3] = {1.0, 0.0, 1.0};
    EXPECT(tgnh_scale_positions(a, nullptr, 0, nullptr) == TGNH_ERR_ARG && tgnh_scale_positions(a, bad, 0, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_scale_positions(a, odd, 1, nullptr) == TGNH_ERR_ARG && tgnh_scale_positions(a, sc, 1, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_restore_positions(a, nullptr) == TGNH_ERR_STATE && tgnh_restore_positions(nullptr, nullptr) == TGNH_ERR_ARG);
    // the periodic box: reduced form or nothing, kept bit for bit; the frame's size; the argument checks before the host-only refusals
    const double ba[3] = {0.83, 0, 0}, bb[3] = {0.17, 0.71, 0}, bc[3] = {-0.29, 0.23, 0.97}, wide[3] = {0.42, 0.71, 0}, tilt[3] = {0.83, 0, 1e-9};
    double ga[3], gb[3], gc[3];
    EXPECT(tgnh_get_periodic_box(a, ga, gb, gc) == TGNH_ERR_STATE && tgnh_wrap_molecules(a, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_set_periodic_box(a, ba, wide, bc) == TGNH_ERR_ARG && tgnh_set_periodic_box(a, tilt, bb, bc) == TGNH_ERR_ARG);
    EXPECT(tgnh_set_periodic_box(a, ba, odd, bc) == TGNH_ERR_ARG && tgnh_set_periodic_box(a, nullptr, bb, bc) == TGNH_ERR_ARG);
    EXPECT(tgnh_get_periodic_box(a, ga, gb, gc) == TGNH_ERR_STATE);
    EXPECT(tgnh_set_periodic_box(a, ba, bb, bc) == TGNH_OK && tgnh_set_periodic_box(a, bb, ba, bc) == TGNH_ERR_ARG);
    EXPECT(tgnh_get_periodic_box(a, ga, gb, gc) == TGNH_OK && tgnh_get_periodic_box(a, nullptr, gb, gc) == TGNH_ERR_ARG);
    for (int k = 0; k < 3; k++) EXPECT(ga[k] == ba[k] && gb[k] == bb[k] && gc[k] == bc[k]);
    int64_t cnt = -1;
    EXPECT(tgnh_get_frame_count(a, 0, &cnt) == TGNH_OK && cnt == N);
    EXPECT(tgnh_get_frame_count(a, TGNH_FRAME_SKIP_DRUDE | TGNH_FRAME_WRAP, &cnt) == TGNH_OK && cnt == N - mols);
    EXPECT(tgnh_get_frame_count(a, 8, &cnt) == TGNH_ERR_ARG && tgnh_get_frame_count(a, 0, nullptr) == TGNH_ERR_ARG && cnt == N - mols);
    float* dev = reinterpret_cast<float*>(4096);                                                               // (never dereferenced: nothing launches)
    tgnh_frame_desc fd{};
    EXPECT(tgnh_write_frame(a, nullptr, dev, nullptr) == TGNH_ERR_ARG && tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_ARG);   // struct_size 0
    fd.struct_size = sizeof(fd); fd.flags = TGNH_FRAME_WRAP | TGNH_FRAME_SKIP_DRUDE; fd.unit = 10.0; fd.stride = N - mols + 7; fd.capacity = 2 * fd.stride + N - mols;
    EXPECT(tgnh_write_frame(a, &fd, nullptr, nullptr) == TGNH_ERR_ARG && tgnh_write_frame(nullptr, &fd, dev, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_STATE);                                          // host-only: nothing launches
    fd.capacity -= 1;
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_ARG);
    fd.capacity += 1; fd.stride = N - mols - 1;
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_ARG);
    fd.flags = TGNH_FRAME_INTERLEAVED; fd.stride = 1; fd.capacity = 3 * N;
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_ARG);
    fd.stride = 0; fd.unit = 0.0;
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_ARG);
    fd.unit = 1.0; fd.flags |= 16;
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_ARG);
    fd.flags = TGNH_FRAME_INTERLEAVED;
    EXPECT(tgnh_write_frame(a, &fd, dev, nullptr) == TGNH_ERR_STATE && tgnh_wrap_molecules(a, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_write_frame(b, &fd, dev, nullptr) == TGNH_ERR_STATE && tgnh_wrap_molecules(nullptr, nullptr) == TGNH_ERR_ARG);
    fd.flags = TGNH_FRAME_WRAP;
    fd.capacity = 3 * N; fd.stride = N;
    EXPECT(tgnh_write_frame(b, &fd, dev, nullptr) == TGNH_ERR_STATE);                                          // b has no box
    // the minimiser: every argument check before the host-only refusal; the mask is never formed, nothing launches, end is harmless
    tgnh_minimize_desc md{};
    md.tolerance = 10.0; md.dt_start = 1e-4; md.dt_max = 1e-3; md.max_step = 0.01; md.f_inc = 1.1; md.f_dec = 0.5; md.alpha_start = 0.1; md.f_alpha = 0.99; md.n_min = 5;
    std::vector<uint8_t> mv(N, 1);
    double* wk = reinterpret_cast<double*>(4096);                                                              // (never dereferenced)
    tgnh_minimize_state ms{};
    EXPECT(tgnh_minimize_begin(a, nullptr, wk, nullptr) == TGNH_ERR_ARG && tgnh_minimize_begin(a, &md, nullptr, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_minimize_begin(nullptr, &md, wk, nullptr) == TGNH_ERR_ARG);
    {
        tgnh_minimize_desc x = md; x.tolerance = -1;    EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.tolerance = NAN;                      EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.dt_start = 0;                         EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.dt_max = 5e-5;                        EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.max_step = INFINITY;                  EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.f_inc = 0.5;                          EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.f_dec = 1.0;                          EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.f_alpha = 0.0;                        EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.alpha_start = 1.5;                    EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.n_min = -1;                           EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.flags = 2;                            EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_ARG);
        x = md; x.flags = TGNH_MIN_DRUDE_ONLY; x.moving = mv.data();
        EXPECT(tgnh_minimize_begin(a, &x, wk, nullptr) == TGNH_ERR_STATE);                                         // host-only: nothing launches
    }
    EXPECT(tgnh_minimize_begin(a, &md, wk, nullptr) == TGNH_ERR_STATE && tgnh_minimize_iterate(a, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_minimize_iterate(nullptr, nullptr) == TGNH_ERR_ARG && tgnh_get_minimize_state(a, nullptr, nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_get_minimize_state(a, nullptr, &ms) == TGNH_ERR_STATE && ms.iterations == 0 && ms.converged == 0);
    EXPECT(tgnh_run_harness_minimize(a, nullptr, 1.0, 1.0, -1, nullptr) == TGNH_ERR_ARG && tgnh_run_harness_minimize(a, nullptr, 1.0, 1.0, 2, nullptr) == TGNH_ERR_STATE);
    EXPECT(tgnh_minimize_end(a) == TGNH_OK && tgnh_minimize_end(a) == TGNH_OK && tgnh_minimize_end(nullptr) == TGNH_ERR_ARG);
    EXPECT(tgnh_destroy(a) == TGNH_OK && tgnh_destroy(b) == TGNH_OK);
    return 0;
}

// invert_shares against its definition: for every slot in ascending order, the (term, role) of its shares in push order
static int inversion_case(const char* name, const std::vector<tgnh::Share>& shares, int slots) {
    const tgnh::ReceiverLists got = tgnh::invert_shares(shares);
    std::vector<int> slot, start, term;
    std::vector<unsigned char> role;
    for (int s = 0; s < slots; s++) {
        const size_t first = term.size();
        for (const tgnh::Share& sh : shares)
            if (sh.slot == s) { term.push_back(sh.term); role.push_back(sh.role); }
        if (term.size() > first) { slot.push_back(s); start.push_back((int)first); }
    }
    start.push_back((int)term.size());
    const char* wrong = term.size() != shares.size() ? "a share outside [0, slots)" : got.slot != slot ? "slot" : got.start != start ? "start" :
                        got.term != term ? "term" : got.role != role ? "role" : nullptr;
    if (wrong) std::fprintf(stderr, "host_driver: invert_shares, %s: %s differs from the restatement\n", name, wrong);
    return wrong ? 1 : 0;
}

static int inversion() {
    const int top = 184;                                          // the highest slot of run()'s handle
    int bad = inversion_case("no share", {}, top + 1);
    bad += inversion_case("one share", {{7, 0, 1}}, top + 1);
    // slot 5 receives from terms 0, 1 and 2, pushed between shares of higher and lower slots
    bad += inversion_case("three terms on a slot", {{9, 0, 0}, {5, 0, 1}, {5, 1, 0}, {2, 1, 1}, {11, 2, 0}, {5, 2, 1}, {0, 2, 2}}, top + 1);
    bad += inversion_case("two shares of a term", {{4, 0, 0}, {3, 0, 1}, {3, 1, 0}, {4, 1, 1}}, top + 1);
    bad += inversion_case("the highest slot", {{top, 0, 0}, {0, 0, 1}, {top, 1, 2}, {top - 1, 1, 0}}, top + 1);
    std::vector<tgnh::Share> many;                                // 300 shares over 64 slots: terms ascending, 1 to 4 shares each, from an LCG
    uint32_t x = 12345;
    auto next = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int t = 0; many.size() < 300; t++)
        for (int m = 0, k = 1 + (int)(next() % 4); m < k; m++) many.push_back({(int)(next() % 64), t, (unsigned char)m});
    bad += inversion_case("300 random shares", many, 64);
    return bad;
}

int main() {
    if (inversion()) return 1;
    if (run(TGNH_MODE_TGNH, 3, 1) || run(TGNH_MODE_DUALNH, 3, 1) || run(TGNH_MODE_DUALNH, 2, 0) || run(TGNH_MODE_TGNH, 1, 1)) return 1;
    std::puts("host_driver: ok");
    return 0;
}
