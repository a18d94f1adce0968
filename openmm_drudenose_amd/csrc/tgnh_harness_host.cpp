// tgnh_harness_host.cpp -- host side of the test force harness (kernels: tgnh_harness.hip): its force, packed / lattice sites, the step loops
#include "tgnh_host.h"

extern "C" tgnh_status tgnh_harness_force(tgnh_handle h, const void* x0, double k_drude, double k_tether,
                                          void* force_out, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    if (!force_out) return fail(TGNH_ERR_ARG, "null force_out");
    if (h->gather.generic) {                                      // the gather path: partners by index (no per-slot word to read an offset from)
        if (!x0) x0 = h->harness.d_g_x0;
        if (!x0) return fail(TGNH_ERR_ARG, "null x0 and no packed sites (tgnh_harness_pack_sites)");
        Timed t(h, (hipStream_t)stream, KID_FORCE);
        HIP_OK(launch_gather_force(h->d.precision, gather_args(h, nullptr), x0, reinterpret_cast<long long*>(force_out), k_drude, k_tether, (hipStream_t)stream));
        return TGNH_OK;
    }
    if (!x0 && !h->harness.d_sflag && !h->harness.lat_on) return fail(TGNH_ERR_ARG, "null x0 and no packed sites (tgnh_harness_pack_sites)");
    ForceArgs a{};
    a.posq = h->bound.posq; a.posq_corr = h->bound.posq_corr; a.x0 = x0; a.meta = h->topo.d_meta;
    if (!x0 && h->harness.lat_on) {
        a.lat_k = h->harness.lat_k; a.lat_side = h->harness.lat_side; a.lat_mol0 = h->harness.lat_mol0; a.lat_spacing = h->harness.lat_spacing; a.lat_tab = h->harness.d_lat_tab;
        a.lat_inv_k = 1.0 / h->harness.lat_k; a.lat_inv_side = 1.0 / h->harness.lat_side; a.lat_inv_side2 = 1.0 / ((double)h->harness.lat_side * h->harness.lat_side);
    } else if (!x0) { a.sflag = h->harness.d_sflag; a.sbase = h->harness.d_sbase; a.sites = h->harness.d_sites; }
    a.force = reinterpret_cast<long long*>(force_out);
    a.n = h->d.num_particles; a.padded = h->d.padded_num_particles;
    a.k_drude = k_drude; a.k_tether = k_tether;
    a.reverse = h->run.sweep_reverse;
    if (h->cfg.alternate_sweeps) h->run.sweep_reverse ^= 1;
    Timed t(h, (hipStream_t)stream, KID_FORCE);
    HIP_OK(launch_force(h->d.precision, a, (hipStream_t)stream));
    return TGNH_OK;
}

// The sites the force kernel needs, without what it does not: x0 spends 16-32 B on every slot for a site only the tethered
// ones have (3 of 5 in SWM4 water), and the meta word 4 B for two bits and a small offset.  Host-side, once.
extern "C" tgnh_status tgnh_harness_pack_sites(tgnh_handle h, const void* x0) {
    tgnh_status rc = entry(h, false); if (rc) return rc;
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle");
    if (!x0) return fail(TGNH_ERR_ARG, "null x0");
    const int N = h->d.num_particles;
    const size_t rs = h->d.precision == TGNH_PREC_DOUBLE ? sizeof(double) : sizeof(float);
    if (h->gather.generic) {                                      // the gather path keeps the sites as they came (its force kernel reads them by index)
        h->harness.lat_on = false;
        if (!h->harness.d_g_x0) HIP_OK(h->harness.d_g_x0.alloc((size_t)std::max(N, 1) * 4 * rs));
        HIP_OK(hipMemcpy(h->harness.d_g_x0, x0, (size_t)N * 4 * rs, hipMemcpyDeviceToDevice));
        return TGNH_OK;
    }
    std::vector<unsigned char> raw((size_t)std::max(N, 1) * 4 * rs);
    HIP_OK(hipMemcpy(raw.data(), x0, (size_t)N * 4 * rs, hipMemcpyDeviceToHost));
    std::vector<uint8_t> flag((size_t)std::max(N, 1), 0);
    std::vector<uint32_t> base((size_t)(N + 63) / 64 + 1, 0);
    std::vector<unsigned char> sites;
    sites.reserve((size_t)N * 3 * rs);
    uint32_t count = 0;
    for (int i = 0; i < N; i++) {
        if ((i & 63) == 0) base[i >> 6] = count;
        const unsigned char* rec = raw.data() + (size_t)i * 4 * rs;
        const bool tethered = rs == sizeof(double) ? reinterpret_cast<const double*>(rec)[3] != 0.0 : reinterpret_cast<const float*>(rec)[3] != 0.0f;
        const uint32_t m = h->topo.meta[i], role = m & 3u;
        const int off = (int)((m >> 10) & 2047u) - 1024;
        const uint32_t o5 = role == ROLE_NORMAL ? 16u : (off >= -15 && off <= 15 ? (uint32_t)(off + 16) : 0u);
        flag[i] = (uint8_t)(role | (tethered && role != ROLE_DRUDE ? 4u : 0u) | (o5 << 3));
        if (flag[i] & 4u) { sites.insert(sites.end(), rec, rec + 3 * rs); count++; }
    }
    h->harness.d_sflag.reset(); h->harness.d_sbase.reset(); h->harness.d_sites.reset();
    h->harness.lat_on = false;
    if (h->harness.lat_k > 0) {
        // The hint (tgnh_harness_lattice_hint) is taken only if it reproduces what was just packed: every slot's byte is molecule
        // 0's, every tethered site is fl(fl64(lattice index x spacing) + geom) in the position type -- the arithmetic of the kernel
        const int k = h->harness.lat_k, side = h->harness.lat_side;
        bool ok = N > 0 && N % k == 0 && (long long)side * side * side >= (long long)h->harness.lat_mol0 + N / k;
        for (int i = 0; i < N && ok; i++) {
            const int pos = i % k, mol = h->harness.lat_mol0 + i / k;
            ok = flag[i] == flag[pos] && (flag[i] >> 3) != 0;         // (a partner more than 15 slots away reads the meta word: not here)
            if (ok && (flag[i] & 4u)) {
                const int idx[3] = {mol / (side * side), (mol / side) % side, mol % side};
                const unsigned char* rec = raw.data() + (size_t)i * 4 * rs;
                for (int ax = 0; ax < 3 && ok; ax++) {
                    volatile double c = (double)idx[ax] * h->harness.lat_spacing;          // (two roundings, as numpy's: no contraction)
                    const double v = c + h->harness.lat_geom[(size_t)pos * 3 + ax];
                    ok = rs == sizeof(double) ? reinterpret_cast<const double*>(rec)[ax] == v : reinterpret_cast<const float*>(rec)[ax] == (float)v;
                }
            }
        }
        if (ok) {
            std::vector<unsigned char> tab(LAT_TAB_BYTES, 0);
            std::memcpy(tab.data(), flag.data(), (size_t)k);
            std::memcpy(tab.data() + 64, h->harness.lat_geom.data(), sizeof(double) * 3 * (size_t)k);
            HIP_OK(h->harness.d_lat_tab.upload(tab));
            h->harness.lat_on = true;
            return TGNH_OK;                                            // nothing per slot is kept
        }
    }
    HIP_OK(h->harness.d_sflag.upload(flag));
    HIP_OK(h->harness.d_sbase.upload(base));
    HIP_OK(h->harness.d_sites.alloc(std::max(sites.size(), (size_t)16) + 16));    // (+16: a 12-byte record may be fetched as four dwords)
    if (!sites.empty()) HIP_OK(hipMemcpy(h->harness.d_sites, sites.data(), sites.size(), hipMemcpyHostToDevice));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_harness_lattice_hint(tgnh_handle h, int mol_slots, int side, double spacing, const double* geom, int first_molecule) {
    CHECK_H(h);
    // a new (or withdrawn) hint is unverified until tgnh_harness_pack_sites has checked it slot by slot: the lattice kernel is
    // not taken with it (tgnh_harness_force with x0 = NULL uses the sites packed before, or fails if there are none)
    h->harness.lat_on = false;
    if (mol_slots == 0) { h->harness.lat_k = 0; h->harness.lat_geom.clear(); return TGNH_OK; }
    if (mol_slots < 1 || mol_slots > 64 || side < 1 || side > 1290 || !(spacing > 0) || !geom || first_molecule < 0) return fail(TGNH_ERR_ARG, "bad lattice hint");
    h->harness.lat_k = mol_slots; h->harness.lat_side = side; h->harness.lat_spacing = spacing; h->harness.lat_mol0 = first_molecule;
    h->harness.lat_geom.assign(geom, geom + 3 * (size_t)mol_slots);
    return TGNH_OK;
}
extern "C" tgnh_status tgnh_harness_sites_kind(tgnh_handle h, int* kind) {
    CHECK_H(h);
    if (!kind) return fail(TGNH_ERR_ARG, "null out");
    *kind = h->harness.lat_on ? 2 : (h->harness.d_sflag ? 1 : 0);
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_run_harness(tgnh_handle h, const void* x0, double k_drude, double k_tether,
                                        int nsteps, void* stream) {
    CHECK_H(h);
    for (int i = 0; i < nsteps; i++) {
        tgnh_status rc = tgnh_step_begin(h, stream); if (rc) return rc;
        rc = tgnh_harness_force(h, x0, k_drude, k_tether, const_cast<void*>(h->bound.force), stream); if (rc) return rc;   // Cu :380 call-out
        rc = tgnh_step_end(h, stream); if (rc) return rc;
    }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_run_steps(tgnh_handle h, int nsteps, void* stream) {
    CHECK_H(h);
    for (int i = 0; i < nsteps; i++) {
        tgnh_status rc = tgnh_step_begin(h, stream); if (rc) return rc;
        rc = tgnh_step_end(h, stream); if (rc) return rc;          // (the force buffer is the caller's business: no call-out here)
    }
    return TGNH_OK;
}
