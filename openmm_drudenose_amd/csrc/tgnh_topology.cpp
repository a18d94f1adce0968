// tgnh_topology.cpp -- topology and tile construction (A1), degrees of freedom and thermostat masses (A2), the upload of their tables
#include <map>

#include "tgnh_host.h"

// ---------------------------------------------------------------------------
// A1 for the gather path (tgnh_gather.hip): the reference's index lists -- normalParticles, pairParticles (Ref :113-137,
// Cu :111-151), particleTempGroup, particleResId, particlesInResidues (Cu :114-125) -- turned per-particle (every particle's pair
// partner | is-Drude << 31, or -1; its group; its residue's index) so that the kernels walk the arrays once, in index order, plus
// the residue table (count, first) and nothing else: no tiles, no per-slot words.  Taken by build_topology for what the tiles
// cannot hold (c->gather.reason says what).
// ---------------------------------------------------------------------------
// per particle: the other member of its pair | is-Drude << 31, -1 in no pair -- from the pair lists build_topology checked
// (the gather kernels' table; the velocity draw's on every handle)
std::vector<int> partner_table(const tgnh_context* c) {
    std::vector<int> t(c->d.num_particles, -1);
    for (size_t k = 0; k < c->topo.pair_drude.size(); k++) {
        const int p = c->topo.pair_drude[k], p1 = c->topo.pair_parent[k];
        t[p] = (int)((unsigned)p1 | 0x80000000u); t[p1] = p;
    }
    return t;
}
// ... on the device, for the passes by global index (GatherArgs::partner): the gather path's own table where the handle has one,
// else one built from the pair lists at the first call and kept.  The handle's device is current (entry).
tgnh_status device_partner_table(tgnh_context* c, const int** out) {
    if (!c->gather.d_partner && !c->by_index.d_partner) HIP_OK(c->by_index.d_partner.upload(partner_table(c)));
    *out = c->gather.d_partner ? c->gather.d_partner : c->by_index.d_partner;
    return TGNH_OK;
}

static tgnh_status build_gather_topology(tgnh_context* c, const std::vector<int>& res_order) {
    const tgnh_desc& d = c->d;
    const int N = d.num_particles;
    const bool com = com_thermostat_on(d);
    c->topo.tile_start.assign(1, N); c->topo.tile_res.assign(1, 0); c->topo.num_tiles = 0;
    c->topo.res_entries.assign(1, make_int2(0, 0));
    c->topo.meta.clear(); c->topo.wave_tile.clear(); c->topo.wmeta.clear(); c->topo.num_wtiles = 0;
    c->topo.tile_pat.assign(1, 0u); c->topo.wtile_pat.assign(1, 0u); c->topo.pattern.assign(PATTERN_WORDS, 0u); c->topo.wpattern.assign(PATTERN_WORDS, 0u);
    c->topo.big_first.clear(); c->topo.big_count.clear(); c->topo.num_big = 0;
    // residues in order of first appearance; a particle's residue as its index in that table
    c->gather.res_table.clear(); c->gather.resid.assign(N, 0);
    if (com) {
        std::vector<int> internal(d.num_residues, -1);
        for (int r : res_order) { internal[r] = (int)c->gather.res_table.size(); c->gather.res_table.push_back(make_int2(c->topo.res_count[r], c->topo.res_first[r])); }
        for (int i = 0; i < N; i++) c->gather.resid[i] = internal[c->topo.resid[i]];
    }
    if (c->gather.res_table.empty()) c->gather.res_table.push_back(make_int2(0, 0));
    {   // gather_com_kernel's lanes per residue: the power of two that holds the mean residue
        const size_t mean = c->gather.res_table.empty() ? 1 : ((size_t)N + c->gather.res_table.size() - 1) / c->gather.res_table.size();
        c->gather.com_lanes = 1;
        while (c->gather.com_lanes < 64 && (size_t)c->gather.com_lanes < mean) c->gather.com_lanes *= 2;
    }
    c->gather.partner = partner_table(c);
    if (c->host_only) return TGNH_OK;
    HIP_OK(c->gather.d_group.upload(c->topo.group));
    HIP_OK(c->gather.d_resid.upload(c->gather.resid));
    HIP_OK(c->gather.d_res_table.upload(c->gather.res_table));
    HIP_OK(c->gather.d_partner.upload(c->gather.partner));
    HIP_OK(c->gather.d_com.alloc(32 * c->gather.res_table.size(), true));          // mixed4 per residue
    // (the tiled path's tables, so that nothing holds a null pointer; no launch of the gather path reads them)
    HIP_OK(c->topo.d_meta.alloc(1));
    HIP_OK(c->topo.d_tile_start.alloc(1));
    HIP_OK(c->topo.d_tile_res.alloc(1));
    HIP_OK(c->topo.d_res_table.alloc(1));
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// A1: topology + tiles
// ---------------------------------------------------------------------------
tgnh_status build_topology(tgnh_context* c, const tgnh_desc* d) {
    const int N = d->num_particles, P = d->num_pairs;
    const bool tg = d->mode == TGNH_MODE_TGNH;
    const bool com = com_thermostat_on(*d);
    c->topo.mass.assign(d->mass, d->mass + N);
    c->topo.pair_drude.assign(d->pair_drude, d->pair_drude + P);
    c->topo.pair_parent.assign(d->pair_parent, d->pair_parent + P);
    // dualNH: the Reference platform never reads getParticleTempGroup (its two thermostats are "everything but the Drude motion" and
    // "the Drude motion", Ref :426-546), so an array handed over in that mode is ignored -- used as it came, its indices sent the
    // kinetic energy of groups 1.. into the unused and the Drude bins of the three-thermostat block (found by tools/fuzz_soak.py --modes)
    if (tg && d->group) c->topo.group.assign(d->group, d->group + N); else c->topo.group.assign(N, 0);
    if (d->resid) c->topo.resid.assign(d->resid, d->resid + N); else c->topo.resid.clear();

    // pair membership; normalParticles = ascending indices in no pair (Ref :113-137, Cu :111-151)
    std::vector<int> role(N, (int)ROLE_NORMAL), partner(N, -1);
    for (int i = 0; i < P; i++) {
        const int p = c->topo.pair_drude[i], p1 = c->topo.pair_parent[i];
        if (p < 0 || p >= N || p1 < 0 || p1 >= N || p == p1) return fail(TGNH_ERR_ARG, "Drude pair index out of range");
        if (partner[p] != -1 || partner[p1] != -1)
            return fail(TGNH_ERR_UNSUPPORTED, "a particle belongs to more than one Drude pair");
        if (c->topo.mass[p] == 0.0 || c->topo.mass[p1] == 0.0)
            return fail(TGNH_ERR_UNSUPPORTED, "massless Drude particle or parent (the reference's pair arithmetic divides by it)");
        role[p] = ROLE_DRUDE; role[p1] = ROLE_PARENT;
        partner[p] = p1; partner[p1] = p;
        if (tg && c->topo.group[p] != c->topo.group[p1])                                // Cu :145-146
            return fail(TGNH_ERR_GROUP_MISMATCH, "Temperature group for drude particle must be the same as the parent particle");
    }
    c->topo.normal.clear();
    for (int i = 0; i < N; i++) if (role[i] == (int)ROLE_NORMAL) c->topo.normal.push_back(i);
    if (tg) {
        for (int i = 0; i < N; i++)
            if (c->topo.group[i] < 0 || c->topo.group[i] >= d->num_groups) return fail(TGNH_ERR_ARG, "temperature group index out of range");
        if (d->num_groups > MAX_GROUPS) {                                     // K :138-200 sizes its bins by G + 2, no limit: the gather path
            c->gather.generic = true; c->gather.reason = "more than 32 temperature groups";
            if (d->num_groups + 2 > GATHER_MAX_NT)
                return fail(TGNH_ERR_UNSUPPORTED, "more than " + std::to_string(GATHER_MAX_NT - 2) + " temperature groups (a wavefront's kinetic-energy bins no longer fit the LDS)");
        }
        for (int i = 0; i < d->num_constraints; i++) {                        // Cu :186-193
            if (!d->constraint_i) break;                                       // (no arrays: every constraint counts against group 0, local_dof_terms)
            const int a = d->constraint_i[i];
            if (a < 0 || a >= N) return fail(TGNH_ERR_ARG, "constraint index out of range");       // (read again by local_dof_terms)
            if (!d->constraint_j) continue;
            const int b = d->constraint_j[i];
            if (b < 0 || b >= N) return fail(TGNH_ERR_ARG, "constraint index out of range");
            if (c->topo.group[a] != c->topo.group[b])
                return fail(TGNH_ERR_GROUP_MISMATCH, "Temperature group of constrained particles must be the same");
        }
    }

    // residue table (count, first) as the reference builds it (Cu :87-89, :119-125)
    const int R = tg ? d->num_residues : 0;
    c->topo.res_count.assign(R, 0);
    c->topo.res_first.assign(R, -1);
    std::vector<int> res_order;        // residues in order of first appearance (internal index)
    std::vector<int> res_internal(R, -1);
    if (tg) {
        if ((int)c->topo.resid.size() != N) return fail(TGNH_ERR_ARG, "TGNH mode needs resid[N]");
        int prev = -1;
        for (int i = 0; i < N; i++) {
            const int r = c->topo.resid[i];
            if (r < 0 || r >= R) return fail(TGNH_ERR_ARG, "residue index out of range");
            c->topo.res_count[r] += 1;
            if (prev != r) {
                // A residue in several runs (e.g. all Drude particles appended behind the atoms): the reference's table still says
                // (count, first) with `first` the start of the LAST run (Cu :121-124) and its COM kernel walks `count` particles
                // from there (K :90-91), whoever they belong to.  The tiles need molecules in one piece; the gather path reproduces
                // that walk as it is (so does the oracle).
                if (com && c->topo.res_first[r] != -1 && !c->gather.generic) { c->gather.generic = true; c->gather.reason = "particles of a residue are not contiguous"; }
                c->topo.res_first[r] = i;
                if (res_internal[r] == -1) { res_internal[r] = (int)res_order.size(); res_order.push_back(r); }
                prev = r;
            }
        }
        if (com) {      // a molecule of massless sites only: the reference forms v_com = 0 * RECIP(0) = NaN for it (K :86-104) and
                        // every thermostat follows; refuse it rather than reproduce that
            std::vector<double> rmass(R, 0.0);
            for (int i = 0; i < N; i++) rmass[c->topo.resid[i]] += c->topo.mass[i];
            for (int r : res_order)
                if (!(rmass[r] > 0.0)) return fail(TGNH_ERR_UNSUPPORTED, "a molecule has no massive particle (its centre-of-mass velocity is undefined)");
        }
    }

    // Molecules longer than a tile ("big": proteins, polymers) cannot have their COM formed in LDS; theirs comes
    // from a table filled by big_com_kernel, and tiles may cut them anywhere (except through a Drude pair).
    std::vector<char> is_big(R, 0);
    c->topo.big_first.clear(); c->topo.big_count.clear();
    std::vector<int> big_index(R, -1);
    if (com) {
        for (int r : res_order) {
            if (c->topo.res_count[r] > TILE_SLOTS) {
                is_big[r] = 1;
                big_index[r] = (int)c->topo.big_first.size();
                c->topo.big_first.push_back(c->topo.res_first[r]);
                c->topo.big_count.push_back(c->topo.res_count[r]);
            }
        }
    }
    // allowed tile cuts: never through a pair, never through a small molecule when the COM is needed
    std::vector<int> forbid(N + 2, 0);
    for (int i = 0; i < P; i++) {
        const int lo = std::min(c->topo.pair_drude[i], c->topo.pair_parent[i]), hi = std::max(c->topo.pair_drude[i], c->topo.pair_parent[i]);
        forbid[lo + 1] += 1; forbid[hi + 1] -= 1;
    }
    if (com) {
        for (int r : res_order) {
            if (is_big[r]) continue;
            // (a residue in several runs -- the gather path, decided above -- has its `count` particles counted from the start of its
            // LAST run: that walk may leave the array; found by tests/test_desc_fuzz.py as a write behind `forbid`)
            const int lo = c->topo.res_first[r], hi = std::min(lo + c->topo.res_count[r] - 1, N - 1);
            forbid[lo + 1] += 1; forbid[hi + 1] -= 1;
        }
    }
    for (int i = 1; i <= N + 1; i++) forbid[i] += forbid[i - 1];
    std::vector<int> res_starts_before(N + 1, 0);      // # residues whose first slot < i
    if (com) {
        std::vector<char> is_start(N, 0);
        for (int r : res_order) is_start[c->topo.res_first[r]] = 1;
        for (int i = 0; i < N; i++) res_starts_before[i + 1] = res_starts_before[i] + is_start[i];
    }
    int align = 1;
#ifdef TGNH_TUNING
    if (const char* e = getenv("TGNH_TILE_ALIGN")) { align = atoi(e); if (align < 1) align = 1; }
#endif
    c->topo.tile_start.clear(); c->topo.tile_res.clear();
    // residues overlapping [start, e): those starting inside, plus one that started before `start`
    auto entries_in = [&](int start, int e) {
        int n = res_starts_before[e] - res_starts_before[start];
        if (start > 0 && start < N && c->topo.resid[start] == c->topo.resid[start - 1]) n += 1;
        return n;
    };
    // Where the molecular COM is not needed (dualNH; TGNH without the COM group) a tile may end inside a molecule -- but a box of
    // one small molecule then has tiles that start at every phase of it, i.e. as many index-word patterns as the molecule has
    // slots, and a kernel whose lane forms its word again for every tile (dualNH/mixed/resident 200 us per launch where TGNH's
    // 60-slot tiles of whole waters take 186).  So a cut that may go anywhere still prefers a molecule's end when one lies within
    // the last tenth of the tile.
    const bool have_resid = (int)c->topo.resid.size() == N;
    auto mol_cut = [&](int st, int end, int span, auto&& legal) {
        if (com || !have_resid || end >= N) return end;
        for (int e = end; e > st && e >= end - span / 10; e--)
            if (c->topo.resid[e] != c->topo.resid[e - 1] && legal(e)) return e;
        return end;
    };
    int cap = TILE_SLOTS;
#ifdef TGNH_TUNING
    if (const char* e = getenv("TGNH_TILE_CAP")) { int v = atoi(e); if (v >= 64 && v <= TILE_SLOTS) cap = v; }
#endif
    int start = 0;
    while (start < N && !c->gather.generic) {
        int end = std::min(start + cap, N);
        auto ok = [&](int e) {
            if (e < N && forbid[e] > 0) return false;
            if (com && entries_in(start, e) > TILE_RES) return false;
            return true;
        };
        while (end > start && !ok(end)) end--;
        if (end == start) {              // no legal cut within a tile's reach: a Drude far from its parent (K :171-186 gathers by arbitrary
            c->gather.generic = true;           // index), or pairs overlapping so densely that no cut between two of them exists -> the gather path
            c->gather.reason = "a Drude pair (or a chain of overlapping pairs) spans more than one 512-slot tile";
            break;
        }
        end = mol_cut(start, end, cap, ok);
        if (align > 1 && end < N) {           // prefer a cut on an `align`-slot boundary close by
            for (int e = end; e > start && e > end - 64; e--)
                if (e % align == 0 && ok(e)) { end = e; break; }
        }
        c->topo.tile_start.push_back(start);
        start = end;
    }
    c->topo.tile_start.push_back(N);
    c->topo.num_tiles = (int)c->topo.tile_start.size() - 1;
    if (c->gather.generic) return build_gather_topology(c, res_order);

    // per-tile residue entries (count, first slot) -- count < 0: big molecule, COM at table index -count-1 --
    // and the packed per-slot words
    std::vector<int2> entries;
    c->topo.tile_res.assign(c->topo.num_tiles + 1, 0);
    c->topo.meta.assign(N, 0);
    for (int t = 0; t < c->topo.num_tiles; t++) {
        c->topo.tile_res[t] = (int)entries.size();
        int prev_res = -1, local = -1;
        for (int i = c->topo.tile_start[t]; i < c->topo.tile_start[t + 1]; i++) {
            if (com && c->topo.resid[i] != prev_res) {
                prev_res = c->topo.resid[i];
                local++;
                entries.push_back(is_big[prev_res] ? make_int2(-(big_index[prev_res] + 1), 0)
                                                   : make_int2(c->topo.res_count[prev_res], c->topo.res_first[prev_res]));
            }
            int off = 0;
            if (partner[i] >= 0) {
                off = partner[i] - i;
                if (partner[i] < c->topo.tile_start[t] || partner[i] >= c->topo.tile_start[t + 1] || off < -1024 || off > 1023)
                    return fail(TGNH_ERR_STATE, "internal: Drude partner outside its tile");
            }
            c->topo.meta[i] = pack_meta((uint32_t)role[i], (uint32_t)c->topo.group[i], off, (uint32_t)(com ? local : 0));
        }
        if (com && local + 1 > TILE_RES) return fail(TGNH_ERR_STATE, "internal: too many molecules in a tile");
    }
    c->topo.tile_res[c->topo.num_tiles] = (int)entries.size();
    if (entries.empty()) entries.push_back(make_int2(0, 0));
    c->topo.res_entries = entries;
    c->topo.num_big = (int)c->topo.big_first.size();

    // Wave tiles for the kinetic-energy passes (wke_kernel, tgnh_internal.h): <= 64 consecutive slots, cut where the
    // 512-slot tiles may be cut (never through a pair, never through a molecule when its COM is needed).  Not possible --
    // a molecule or a pair longer than a wavefront -- leaves the list empty and the KE passes on the tile kernel.
    c->topo.wave_tile.clear(); c->topo.wmeta.clear(); c->topo.num_wtiles = 0;
    if (c->topo.num_big == 0) {
        std::vector<int2> wt;
        bool fits = true;
        for (int st = 0; st < N && fits;) {
            int end = std::min(st + WAVE_SLOTS, N);
            while (end > st && end < N && forbid[end] > 0) end--;
            if (end == st) { fits = false; break; }
            end = mol_cut(st, end, WAVE_SLOTS, [&](int e) { return forbid[e] == 0; });
            int maxn = 1;
            if (com) for (int i = st; i < end; i++) maxn = std::max(maxn, c->topo.res_count[c->topo.resid[i]]);
            wt.push_back(make_int2(st, maxn));
            st = end;
        }
        if (fits) {
            c->topo.num_wtiles = (int)wt.size();
            wt.push_back(make_int2(N, 0));
            c->topo.wmeta.assign(N, 0);
            for (int i = 0; i < N; i++) {
                int pos = 0, n = 1;
                if (com) { const int r = c->topo.resid[i]; pos = i - c->topo.res_first[r]; n = c->topo.res_count[r]; }
                const int off = partner[i] >= 0 ? partner[i] - i : 0;    // inside the wave tile: no cut goes through a pair
                c->topo.wmeta[i] = pack_wmeta((uint32_t)role[i], (uint32_t)c->topo.group[i], off, (uint32_t)pos, (uint32_t)(n - 1));
            }
            c->topo.wave_tile = wt;
        }
    }
    // tiles of identical molecules (PATTERN_WORDS, tgnh_internal.h)
    {
        std::map<std::vector<uint32_t>, uint32_t> ids, wids;
        // mass != nullptr: the key is the P words AND the P descriptor masses behind them (the wave tiles: two tiles share a
        // pattern only if their masses agree too -- a pattern then has ONE table of inverse masses, wpat_mass, for the one-launch
        // step's velocity planes); known_only: an id is handed out only for a pattern some earlier tile has made
        auto intern = [&](std::map<std::vector<uint32_t>, uint32_t>& m, std::vector<uint32_t>& store, const uint32_t* w, int P,
                          uint32_t limit, uint32_t* id, const double* mass = nullptr, bool known_only = false) {
            std::vector<uint32_t> key(w, w + P);
            if (mass) { key.resize(3 * (size_t)P); std::memcpy(key.data() + P, mass, sizeof(double) * P); }
            auto it = m.find(key);
            if (it == m.end()) {
                if (known_only || m.size() >= limit) return false;
                it = m.emplace(key, (uint32_t)m.size()).first;
                std::vector<uint32_t> words(w, w + P);
                words.resize(PATTERN_WORDS, 0u);
                store.insert(store.end(), words.begin(), words.end());
                if (mass) { c->topo.wpat_mass.insert(c->topo.wpat_mass.end(), mass, mass + P); c->topo.wpat_mass.resize(store.size(), 0.0); }
            }
            *id = it->second;
            return true;
        };
        c->topo.tile_pat.assign(std::max(c->topo.num_tiles, 1), 0u); c->topo.pattern.clear();
        for (int t = 0; t < c->topo.num_tiles; t++) {
            const int ts = c->topo.tile_start[t], n = c->topo.tile_start[t + 1] - ts;
            // the smallest period that reproduces the tile (a wrong one fails within a few slots); the molecules it spans are
            // read off the molecule index of the slot one period in (a cation and its anion: 2; ten waters, one tagged: 10)
            for (int P = 1; P <= PATTERN_WORDS && P < n; P++) {
                const uint32_t mols = com ? (c->topo.meta[ts + P] >> 21) - (c->topo.meta[ts] >> 21) : 0u;
                if (mols > 255u) break;
                bool same = true;
                for (int k = 0; k < n && same; k++)
                    same = c->topo.meta[ts + k] == c->topo.meta[ts + k % P] + (((uint32_t)(k / P) * mols) << 21);
                if (!same) continue;
                uint32_t id;
                if (intern(ids, c->topo.pattern, c->topo.meta.data() + ts, P, 1u << 16, &id))
                    c->topo.tile_pat[t] = (uint32_t)P | (mols << 8) | (id << 16);
                break;
            }
        }
        c->topo.wtile_pat.assign(std::max(c->topo.num_wtiles, 1), 0u); c->topo.wpattern.clear(); c->topo.wpat_mass.clear();
        c->topo.wpat_all_uniform = c->topo.num_wtiles > 0;
        for (int t = 0; t < c->topo.num_wtiles; t++) {
            const int ws = c->topo.wave_tile[t].x, n = c->topo.wave_tile[t + 1].x - ws;
            // (P == n: a tile of one period -- the single molecule a box ends with -- takes the pattern the tiles before it made)
            for (int P = 1; P <= PATTERN_WORDS && P <= n; P++) {
                bool same = true;
                for (int k = 0; k < n && same; k++) same = c->topo.wmeta[ws + k] == c->topo.wmeta[ws + k % P];
                if (!same) continue;
                uint32_t id;
                if (intern(wids, c->topo.wpattern, c->topo.wmeta.data() + ws, P, 1u << 16, &id, c->topo.mass.data() + ws, P == n)) {
                    c->topo.wtile_pat[t] = (uint32_t)P | (id << 8);
                    // the words repeat with period P; do the masses?  (bit for bit: what the pattern's table of inverse masses stands for)
                    for (int k = 0; k < n; k++)
                        if (std::memcmp(&c->topo.mass[ws + k], &c->topo.wpat_mass[(size_t)id * PATTERN_WORDS + k % P], sizeof(double))) c->topo.wpat_all_uniform = false;
                }
                break;
            }
            if (!c->topo.wtile_pat[t]) c->topo.wpat_all_uniform = false;
        }
        // Where the velocity planes keep a slot (tgnh_context.h Topology::wtile_base, wpat_off): the massive slots only, packed in
        // slot order, every tile's segment on a 128-byte line of the plane (16 words of 8 bytes: the planes exist in mixed and
        // double precision).  A lane's offset counts the massive slots of its tile before it: a function of pattern and lane.
        c->topo.wtile_base.clear(); c->topo.wpat_off.clear();
        if (c->topo.wpat_all_uniform) {
            const size_t patterns = c->topo.wpattern.size() / PATTERN_WORDS;
            std::vector<char> made(patterns, 0);
            c->topo.wpat_off.assign(patterns * PATTERN_WORDS, 0u);
            c->topo.wtile_base.assign((size_t)c->topo.num_wtiles + 1, 0u);
            uint64_t base = 0;
            for (int t = 0; t < c->topo.num_wtiles; t++) {
                const int ws = c->topo.wave_tile[t].x, n = c->topo.wave_tile[t + 1].x - ws;
                const uint32_t P = c->topo.wtile_pat[t] & 255u, id = c->topo.wtile_pat[t] >> 8;
                if (!made[id]) {
                    uint32_t before = 0;
                    for (uint32_t lane = 0; lane < (uint32_t)PATTERN_WORDS; lane++) {
                        c->topo.wpat_off[(size_t)id * PATTERN_WORDS + lane] = before;
                        before += c->topo.wpat_mass[(size_t)id * PATTERN_WORDS + lane % P] != 0.0;
                    }
                    made[id] = 1;
                }
                uint32_t massive = 0;
                for (int k = 0; k < n; k++) massive += c->topo.mass[ws + k] != 0.0;
                c->topo.wtile_base[t] = (uint32_t)base;
                base = (base + massive + 15u) & ~(uint64_t)15u;
            }
            c->topo.wtile_base[c->topo.num_wtiles] = (uint32_t)base;
            // (the kernels index the third plane with an int, as they index the force buffer's)
            if (3 * base > (uint64_t)INT32_MAX) { c->topo.wtile_base.clear(); c->topo.wpat_off.clear(); }
        }
        if (c->topo.pattern.empty()) c->topo.pattern.assign(PATTERN_WORDS, 0u);
        if (c->topo.wpattern.empty()) c->topo.wpattern.assign(PATTERN_WORDS, 0u);
    }
    if (c->host_only) return TGNH_OK;
    // device copies
    HIP_OK(c->topo.d_tile_pat.upload(c->topo.tile_pat));
    HIP_OK(c->topo.d_pattern.upload(c->topo.pattern));
    HIP_OK(c->topo.d_wpattern.upload(c->topo.wpattern));
    HIP_OK(c->topo.d_meta.upload(c->topo.meta));
    HIP_OK(c->topo.d_tile_start.upload(c->topo.tile_start));
    HIP_OK(c->topo.d_tile_res.upload(c->topo.tile_res));
    HIP_OK(c->topo.d_res_table.upload(c->topo.res_entries));
    if (!c->topo.wave_tile.empty()) {
        std::vector<int2> packed = c->topo.wave_tile;           // device copy: y = largest molecule | period << 8 | pattern << 16
        for (int t = 0; t < c->topo.num_wtiles; t++) packed[t].y |= (int)(c->topo.wtile_pat[t] << 8);
        HIP_OK(c->topo.d_wave_tile.upload(packed));
        HIP_OK(c->topo.d_wmeta.upload(c->topo.wmeta));
    }
    if (c->topo.num_big) {
        std::vector<int2> bt(c->topo.num_big);
        for (int k = 0; k < c->topo.num_big; k++) bt[k] = make_int2(c->topo.big_count[k], c->topo.big_first[k]);
        HIP_OK(c->topo.d_big_table.upload(bt));
        HIP_OK(c->topo.d_big_com.alloc(32 * (size_t)c->topo.num_big, true));           // mixed4 per big molecule
    }
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// A2: degrees of freedom (additive local terms) and thermostat block
// ---------------------------------------------------------------------------
void local_dof_terms(tgnh_context* c) {
    const tgnh_desc& d = c->d;
    const int N = d.num_particles, P = d.num_pairs;
    const int NT = c->thermo.L.NT;
    c->thermo.local_terms.assign(NT, 0.0);
    if (d.mode == TGNH_MODE_DUALNH) {
        double real = 0;
        for (int i = 0; i < N; i++) real += (c->topo.mass[i] == 0.0 ? 0 : 3);      // Ref :119
        real -= 3.0 * P;                                                      // Ref :133
        real -= d.num_constraints;                                            // Ref :157
        c->thermo.local_terms[0] = real;
        c->thermo.local_terms[2] = 3.0 * P;                                          // Ref :134
        return;
    }
    const int G = d.num_groups, R = d.num_residues;
    std::vector<double> resInv(R, 0.0);                                       // API :147-153
    {
        std::vector<double> rm(R, 0.0);
        for (int i = 0; i < N; i++) rm[c->topo.resid[i]] += c->topo.mass[i];
        for (int r = 0; r < R; r++) resInv[r] = 1.0 / rm[r];
    }
    std::vector<double> dof(G, 0.0), red(G, 0.0);
    for (int i = 0; i < N; i++) {                                             // Cu :126-133
        if (c->topo.mass[i] != 0.0) {
            dof[c->topo.group[i]] += 3;
            if (d.use_com_temp_group) red[c->topo.group[i]] += 3 * c->topo.mass[i] * resInv[c->topo.resid[i]];
        }
    }
    for (int i = 0; i < P; i++) dof[c->topo.group[c->topo.pair_drude[i]]] -= 3;         // Cu :148
    for (int i = 0; i < d.num_constraints; i++) {                             // Cu :195
        if (d.constraint_i) dof[c->topo.group[d.constraint_i[i]]] -= 1; else dof[0] -= 1;
    }
    for (int g = 0; g < G; g++) c->thermo.local_terms[g] = dof[g] - red[g];          // Cu :219
    c->thermo.local_terms[G] = d.use_com_temp_group ? 3.0 * R : 0.0;                 // Cu :197-199
    c->thermo.local_terms[G + 1] = 3.0 * P;                                          // Cu :149, :201
}

// The two bath temperatures of a handle: tgnh_create's, and tgnh_set_temperatures' later.  (OpenMM's setTemperature checks
// nothing and neither does tgnh_create; the setter of a live handle and the velocity draw refuse what cannot be a temperature.)
tgnh_status check_temperatures(double temperature, double drude_temperature) {
    if (!(temperature >= 0) || !std::isfinite(temperature) || !(drude_temperature >= 0) || !std::isfinite(drude_temperature))
        return fail(TGNH_ERR_ARG, "a temperature must be finite and not negative");
    return TGNH_OK;
}
void set_bath_temperatures(tgnh_context* c, double temperature, double drude_temperature) {
    c->d.temperature = temperature; c->d.drude_temperature = drude_temperature;      // (the hard wall's thermal speed reads the latter)
    c->thermo.realkbT = c->d.kB * temperature;                                       // Ref :107-108, Cu :80-81
    c->thermo.drudekbT = c->d.kB * drude_temperature;
}

// Every thermostat's N kT from thermo.dof and a pair of kT: what computes, apart from what stores.  thermostat_targets keeps the
// result for the handle's own baths; tgnh_rescale_to_temperature asks for other temperatures' and leaves the baths alone.
std::vector<double> thermostat_nkt(const tgnh_context* c, double realkbT, double drudekbT) {
    const ChainLayout& L = c->thermo.L;
    std::vector<double> nkbt(L.NT, 0.0);
    if (c->d.mode == TGNH_MODE_DUALNH) {
        nkbt[0] = c->thermo.dof[0] * realkbT; nkbt[2] = c->thermo.dof[2] * drudekbT;      // Ref :168-169
    } else {
        for (int i = 0; i < L.G + 1; i++) nkbt[i] = c->thermo.dof[i] * realkbT;           // Cu :218-225
        nkbt[L.G + 1] = c->thermo.dof[L.G + 1] * drudekbT;                                // Cu :227-235
    }
    return nkbt;
}

// What the bath temperatures decide of the thermostat block -- every N kT (thermo.nkbt too) and every thermostat mass, and the
// etaDotDot a chain STARTS with -- written into st (the block's layout, zero elsewhere) from thermo.dof and kT, kT_D.
void thermostat_targets(tgnh_context* c, std::vector<double>& st) {
    const tgnh_desc& d = c->d;
    const ChainLayout& L = c->thermo.L;
    const int NT = L.NT, C = L.C;
    c->thermo.nkbt = thermostat_nkt(c, c->thermo.realkbT, c->thermo.drudekbT);
    const double tau2 = std::pow(d.coupling_time, 2), tauD2 = std::pow(d.drude_coupling_time, 2);
    if (d.mode == TGNH_MODE_DUALNH) {
        const double realNkbT = c->thermo.nkbt[0], drudeNkbT = c->thermo.nkbt[2];
        double* etaMass = st.data() + L.off_etaMass;
        double* etaDot = st.data() + L.off_etaDot;
        double* etaDotDot = st.data() + L.off_etaDotDot;
        etaMass[0] = realNkbT * tau2;                                         // Ref :170-171
        etaMass[1] = drudeNkbT * tauD2;
        const int ntg = L.numTempGroup;
        if (L.use_drude_chains) {                                             // Ref :192-205
            for (int ich = 1; ich < C; ich++) {
                etaMass[2 * ich] = c->thermo.realkbT * tau2;
                etaMass[2 * ich + 1] = c->thermo.drudekbT * tauD2;
                etaDotDot[ich * ntg] = (etaMass[(ich - 1) * ntg] * etaDot[(ich - 1) * ntg] * etaDot[(ich - 1) * ntg] - c->thermo.realkbT) / etaMass[ich * ntg];
                etaDotDot[ich * ntg + 1] = (etaMass[(ich - 1) * ntg + 1] * etaDot[(ich - 1) * ntg + 1] * etaDot[(ich - 1) * ntg + 1] - c->thermo.drudekbT) / etaMass[ich * ntg + 1];
            }
        } else {                                                              // Ref :206-214
            for (int ich = 1; ich < C; ich++) {
                etaMass[ich + 1] = c->thermo.realkbT * tau2;
                etaDotDot[ich * ntg + 1] = (etaMass[(ich - 1) * ntg + 1] * etaDot[(ich - 1) * ntg + 1] * etaDot[(ich - 1) * ntg + 1] - c->thermo.realkbT) / etaMass[ich * ntg + 1];
            }
        }
    } else {
        const int G = L.G;
        const double realUnit = c->thermo.realkbT * tau2, drudeUnit = c->thermo.drudekbT * tauD2;   // Cu :216-217
        for (int i = 0; i < G + 1; i++) {                                     // Cu :218-225
            double* em = st.data() + L.off_etaMass + i * C;
            double* edd = st.data() + L.off_etaDotDot + i * C;
            em[0] = c->thermo.dof[i] * realUnit;
            for (int ich = 1; ich < C; ich++) { em[ich] = realUnit; edd[ich] = (em[ich - 1] * 0.0 - c->thermo.realkbT) / em[ich]; }
        }
        const int itg = G + 1;                                                // Cu :227-235
        double* em = st.data() + L.off_etaMass + itg * C;
        double* edd = st.data() + L.off_etaDotDot + itg * C;
        em[0] = c->thermo.dof[itg] * drudeUnit;
        for (int ich = 1; ich < C; ich++) {
            em[ich] = drudeUnit;
            if (L.use_drude_chains) edd[ich] = (em[ich - 1] * 0.0 - c->thermo.drudekbT) / em[ich];
        }
    }
    for (int i = 0; i < NT; i++) st[L.off_nkbt + i] = c->thermo.nkbt[i];
}

tgnh_status finalize_thermostat(tgnh_context* c) {
    const tgnh_desc& d = c->d;
    ChainLayout& L = c->thermo.L;
    const int NT = L.NT;
    c->thermo.dof = c->thermo.global_terms;
    if (d.has_cm_motion_remover) {
        if (d.mode == TGNH_MODE_DUALNH) c->thermo.dof[0] -= 3;                       // Ref :158-165
        else if (d.use_com_temp_group) c->thermo.dof[L.G] -= 3;                      // Cu :204-212
    }
    std::vector<double> st(L.total, 0.0);
    thermostat_targets(c, st);
    for (int i = 0; i < NT; i++) {
        st[L.off_scale + i] = 1.0; st[L.off_scale_a + i] = 1.0; st[L.off_scale_b + i] = 1.0;
    }
    c->thermo.h_state = st;
    if (!c->host_only) {
        HIP_OK(hipMemcpy(c->thermo.d_state, st.data(), sizeof(double) * L.total, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(c->thermo.d_stage, st.data(), sizeof(double) * L.total, hipMemcpyHostToDevice));
    }
    c->owed.thermostat_reset();
    return TGNH_OK;
}

void make_layout(tgnh_context* c) {
    const tgnh_desc& d = c->d;
    ChainLayout& L = c->thermo.L;
    L.mode = d.mode;
    L.C = d.num_nh_chains;
    L.use_drude_chains = d.use_drude_nh_chains ? 1 : 0;
    if (d.mode == TGNH_MODE_DUALNH) {
        L.G = 1; L.NT = 3;
        const int C = L.C;
        if (L.use_drude_chains) { L.numTempGroup = 2; L.idxMaxNHChains = 2 * C - 1; L.iNumNHChains = 2 * C; }   // Ref :139-154
        else { L.numTempGroup = 1; L.idxMaxNHChains = C; L.iNumNHChains = C + 1; }
        const int n = L.use_drude_chains ? 2 * C : C + 1;
        L.len_eta = n; L.len_etaDotDot = n; L.len_etaMass = n; L.len_etaDot = n + 2;          // Ref :216-217
        L.c1_shift = 1; L.c1_mul = 1; L.c1_add = 2; L.c1_unused = 1; L.c1_guard_below = 0;
        L.c1_quirk = L.use_drude_chains ? 0 : 1;
    } else {
        L.G = d.num_groups; L.NT = L.G + 2;
        L.len_eta = L.NT * L.C; L.len_etaDotDot = L.NT * L.C; L.len_etaMass = L.NT * L.C;     // Cu :94-97
        L.len_etaDot = L.NT * (L.C + 1);
        L.numTempGroup = L.idxMaxNHChains = L.iNumNHChains = 0;
        L.c1_shift = 0; L.c1_mul = 2; L.c1_add = 1; L.c1_unused = -1; L.c1_guard_below = L.NT - 1;
        L.c1_quirk = 0;
    }
    int o = 0;
    L.off_eta = o; o += L.len_eta;
    L.off_etaDot = o; o += L.len_etaDot;
    L.off_etaDotDot = o; o += L.len_etaDotDot;
    L.off_etaMass = o; o += L.len_etaMass;
    L.off_nkbt = o; o += L.NT;
    L.off_ke = o; o += L.NT;
    o = (o + 1) & ~1;                         // 16-byte aligned: this one is handed to the all-reduce hook
    L.off_ke_red = o; o += L.NT;
    L.off_scale = o; o += L.NT;
    L.off_scale_a = o; o += L.NT;
    L.off_scale_b = o; o += L.NT;
    L.off_kesum = o; o += 1;
    L.off_ke_post = o; o += L.NT;
    L.total = o;
}
