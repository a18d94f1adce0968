// tgnh_positions.cpp -- the molecule table (labels, pair check, spans and member lists, eligibility for the span kernel), tgnh_scale_positions and its snapshot, tgnh_restore_positions
// (tgnh_frames.cpp has the table's other user: the periodic box, tgnh_wrap_molecules, tgnh_write_frame)
#include <unordered_map>

#include "tgnh_host.h"

// ---------------------------------------------------------------------------
// the molecule table (include/drude_tgnh.h has the contract)
// ---------------------------------------------------------------------------
// labels -> 0..M-1 in order of first appearance
static int renumber(const int32_t* label, int N, std::vector<int>& mol_of) {
    mol_of.resize(N);
    int32_t lo = label[0], hi = label[0];
    for (int i = 1; i < N; i++) { lo = std::min(lo, label[i]); hi = std::max(hi, label[i]); }
    const long long range = (long long)hi - lo + 1;
    int M = 0;
    if (range <= 4LL * N + 1024) {                              // (residue indices and the like: a direct table)
        std::vector<int> seen((size_t)range, -1);
        for (int i = 0; i < N; i++) {
            int& m = seen[(size_t)((long long)label[i] - lo)];
            if (m < 0) m = M++;
            mol_of[i] = m;
        }
    } else {
        std::unordered_map<int32_t, int> seen;
        for (int i = 0; i < N; i++) {
            auto it = seen.find(label[i]);
            if (it == seen.end()) it = seen.emplace(label[i], M++).first;
            mol_of[i] = it->second;
        }
    }
    return M;
}

// Everything the table is, from the labels; the handle's table is replaced only when all of it stands.
static tgnh_status molecules_build(tgnh_context* c, const int32_t* label, const char* what) {
    const int N = c->d.num_particles;
    tgnh_context::Molecules::Table m;
    m.count = renumber(label, N, m.mol_of);
    for (size_t k = 0; k < c->topo.pair_drude.size(); k++) {
        const int d = c->topo.pair_drude[k], p = c->topo.pair_parent[k];
        if (m.mol_of[d] != m.mol_of[p])
            return fail(TGNH_ERR_ARG, std::string(what) + ": Drude pair " + std::to_string(k) + " (Drude particle " + std::to_string(d) + ", parent " +
                                      std::to_string(p) + ") lies in two molecules: the move would stretch its spring");
    }
    // member lists: the slots by molecule, ascending within one (a counting sort keeps the slot order)
    m.mem_start.assign((size_t)m.count + 1, 0);
    for (int i = 0; i < N; i++) m.mem_start[m.mol_of[i] + 1]++;
    for (int k = 0; k < m.count; k++) m.mem_start[k + 1] += m.mem_start[k];
    m.members.resize(N);
    {
        std::vector<int> at(m.mem_start.begin(), m.mem_start.end() - 1);
        for (int i = 0; i < N; i++) m.members[at[m.mol_of[i]]++] = i;
    }
    // the span kernel serves a table in which every molecule is a run of consecutive slots no longer than a wavefront: numbered by
    // first appearance, such molecules are the member lists themselves (members[i] == i)
    m.spans = true;
    for (int k = 0; k < m.count && m.spans; k++) {
        const int b = m.mem_start[k], n = m.mem_start[k + 1] - b;
        if (n > SP_SPAN_SLOTS || m.members[b] != b || m.members[b + n - 1] != b + n - 1) m.spans = false;
    }
    if (m.spans) {       // spans of whole molecules, <= 64 slots, cut greedily; bit l of a span's heads: a molecule starts at its lane l
        for (int k = 0; k < m.count; k++) {
            const int b = m.mem_start[k], e = m.mem_start[k + 1];
            if (m.span_first.empty() || e - m.span_first.back() > SP_SPAN_SLOTS) { m.span_first.push_back(b); m.span_heads.push_back(0ull); }
            m.span_heads.back() |= 1ull << (b - m.span_first.back());
        }
        m.span_first.push_back(N);
        // a frame without Drude slots: where a span's kept slots start in the output, and which of its lanes are left out
        std::vector<char> drude((size_t)N, 0);
        for (int d : c->topo.pair_drude) drude[d] = 1;
        int kept = 0;
        for (size_t k = 0; k + 1 < m.span_first.size(); k++) {
            unsigned long long mask = 0ull;
            m.span_out.push_back(kept);
            for (int i = m.span_first[k]; i < m.span_first[k + 1]; i++) {
                if (drude[i]) mask |= 1ull << (i - m.span_first[k]);
                else kept++;
            }
            m.span_drude.push_back(mask);
        }
    }
    c->mol.drop_device();                // (the old table's device copies; the next launching call uploads these: the caller has made the device current)
    c->mol.t = std::move(m);
    c->mol.set = true;
    return TGNH_OK;
}

// the table in force: the caller's, or the default (the descriptor's resid) resolved at the first call that needs one
tgnh_status molecules_ensure(tgnh_context* c, const char* what) {
    if (c->mol.set) return TGNH_OK;
    if ((int)c->topo.resid.size() != c->d.num_particles)
        return fail(TGNH_ERR_STATE, std::string(what) + ": the handle was created without resid, so there is no default molecule table: call tgnh_set_molecules first");
    return molecules_build(c, c->topo.resid.data(), what);
}

// device copies of the tables the launches read, made once per table (never inside a stream capture: the uploads are synchronous)
tgnh_status molecules_device(tgnh_context* c, hipStream_t s) {
    tgnh_context::Molecules& m = c->mol;
    if (m.on_device) return TGNH_OK;
    const tgnh_context::Molecules::Table& t = m.t;
    if (stream_capturing(s)) return fail(TGNH_ERR_STATE, "tgnh_scale_positions: the molecule tables are not on the device yet and the stream is capturing "
                                         "(call tgnh_set_molecules or tgnh_scale_positions once outside the capture)");
    if (t.spans) {
        // (once per table, not per call: every span a wavefront's, its first lane a molecule's head)
        for (size_t k = 0; k + 1 < t.span_first.size() && k < t.span_heads.size(); k++)
            if (t.span_first[k + 1] - t.span_first[k] < 1 || t.span_first[k + 1] - t.span_first[k] > SP_SPAN_SLOTS || !(t.span_heads[k] & 1ull))
                return fail(TGNH_ERR_STATE, "internal: a span longer than a wavefront");
        HIP_OK(m.d_span_first.upload(t.span_first));
        HIP_OK(m.d_span_heads.upload(t.span_heads));
        HIP_OK(m.d_span_out.upload(t.span_out));
        HIP_OK(m.d_span_drude.upload(t.span_drude));
    } else {
        HIP_OK(m.d_mol_of.upload(t.mol_of));
        HIP_OK(m.d_mem_start.upload(t.mem_start));
        HIP_OK(m.d_members.upload(t.members));
        HIP_OK(m.d_shift.alloc(3 * (size_t)t.count));            // (every entry is written by the first launch before the second reads it)
    }
    m.on_device = true;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_molecules(tgnh_handle h, const int32_t* molecule) {
    CHECK_H(h);
    if (!h->host_only) HIP_OK(hipSetDevice(h->device));          // (the old device tables are released here)
    tgnh_status rc;
    if (molecule) rc = molecules_build(h, molecule, "tgnh_set_molecules");
    else if ((int)h->topo.resid.size() != h->d.num_particles)
        rc = fail(TGNH_ERR_STATE, "tgnh_set_molecules: the handle was created without resid, so there is no default molecule table");
    else rc = molecules_build(h, h->topo.resid.data(), "tgnh_set_molecules");
    if (rc) return rc;
    return h->host_only ? TGNH_OK : molecules_device(h, nullptr);
}

extern "C" tgnh_status tgnh_get_num_molecules(tgnh_handle h, int* count) {
    CHECK_H(h);
    if (!count) return fail(TGNH_ERR_ARG, "null count");
    tgnh_status rc = molecules_ensure(h, "tgnh_get_num_molecules"); if (rc) return rc;
    *count = h->mol.t.count;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_molecules(tgnh_handle h, int32_t* molecule_out) {
    CHECK_H(h);
    if (!molecule_out) return fail(TGNH_ERR_ARG, "null molecule_out");
    tgnh_status rc = molecules_ensure(h, "tgnh_get_molecules"); if (rc) return rc;
    std::copy(h->mol.t.mol_of.begin(), h->mol.t.mol_of.end(), molecule_out);
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// tgnh_scale_positions / tgnh_restore_positions (tgnh_scale_positions.hip has the kernels)
// ---------------------------------------------------------------------------
static size_t posq_bytes(const tgnh_context* c) { return (size_t)c->d.num_particles * (c->d.precision == TGNH_PREC_DOUBLE ? 32 : 16); }
static size_t corr_bytes(const tgnh_context* c) { return c->d.precision == TGNH_PREC_MIXED ? (size_t)c->d.num_particles * 16 : 0; }

// what the launches are bound by, against what the tables hold: a launch that would run off a buffer is not made
tgnh_status molecules_launch_bounds(const tgnh_context* c) {
    const tgnh_context::Molecules& m = c->mol;
    const tgnh_context::Molecules::Table& t = m.t;
    const int N = c->d.num_particles;
    if (!m.set || !m.on_device || t.count < 1 || t.count > N || (int)t.mol_of.size() != N)
        return fail(TGNH_ERR_STATE, "internal: the molecule table does not match the handle");
    if (t.spans) {
        const size_t ns = t.span_heads.size();
        if (ns < 1 || t.span_first.size() != ns + 1 || t.span_first.front() != 0 || t.span_first.back() != N || !m.d_span_first || !m.d_span_heads ||
            t.span_out.size() != ns || t.span_drude.size() != ns || !m.d_span_out || !m.d_span_drude)
            return fail(TGNH_ERR_STATE, "internal: the span table does not cover the slots");
    } else if ((int)t.members.size() != N || (int)t.mem_start.size() != t.count + 1 || t.mem_start.back() != N || !m.d_mol_of || !m.d_mem_start ||
               !m.d_members || !m.d_shift)
        return fail(TGNH_ERR_STATE, "internal: the member table does not cover the slots");
    if (c->d.precision == TGNH_PREC_MIXED && !c->bound.posq_corr) return fail(TGNH_ERR_STATE, "internal: mixed precision without a position correction");
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_scale_positions(tgnh_handle h, const double scale[3], int save, void* stream) {
    CHECK_H(h);
    if (!scale) return fail(TGNH_ERR_ARG, "tgnh_scale_positions: null scale");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(scale[k]) || !(scale[k] > 0.0)) return fail(TGNH_ERR_ARG, "tgnh_scale_positions: a scale factor is not finite or not positive");
    tgnh_status rc = entry(h, true); if (rc) return rc;           // (buffers bound, not a host-only handle, no failure seen before)
    hipStream_t s = (hipStream_t)stream;
    rc = molecules_ensure(h, "tgnh_scale_positions"); if (rc) return rc;
    // bits 0 and 2 of tgnh_get_pending_state: a half kick is still owed to velm.  It belongs to the forces of the positions as they
    // are; the folded launch of the next tgnh_step_begin would take it from the forces of the moved ones.
    if (h->owed.end_pending || h->owed.kick_pending)
        return fail(TGNH_ERR_STATE, "tgnh_scale_positions: a half kick of the last step is still owed to the velocities (tgnh_flush first)");
    rc = molecules_device(h, s); if (rc) return rc;
    tgnh_context::PositionSnapshot& snap = h->snap;
    if (save && !snap.d_posq) {                                  // one copy of the positions, allocated at the first saving call
        HIP_OK(snap.d_posq.alloc(posq_bytes(h)));
        if (corr_bytes(h)) HIP_OK(snap.d_corr.alloc(corr_bytes(h)));
    }
    rc = molecules_launch_bounds(h); if (rc) return rc;
    const tgnh_context::Molecules& m = h->mol;
    ScalePosArgs a{};
    a.posq = h->bound.posq; a.corr = h->bound.posq_corr; a.n = h->d.num_particles;
    if (save) { a.snap_posq = snap.d_posq; a.snap_corr = snap.d_corr; }
    for (int k = 0; k < 3; k++) a.sm1[k] = scale[k] - 1.0;
    a.num_molecules = m.t.count;
    Timed t(h, s, KID_OTHER);
    if (m.t.spans) {
        a.span_first = m.d_span_first; a.span_heads = m.d_span_heads; a.num_spans = (int)m.t.span_heads.size();
        HIP_OK(launch_scale_positions_spans(h->d.precision, a, s));
    } else {
        a.mol_of = m.d_mol_of; a.mem_start = m.d_mem_start; a.members = m.d_members; a.shift = m.d_shift;
        HIP_OK(launch_scale_positions_table(h->d.precision, a, s));
    }
    if (save) { snap.taken = snap.valid = true; snap.of_posq = h->bound.posq; snap.of_corr = h->bound.posq_corr; }
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_restore_positions(tgnh_handle h, void* stream) {
    tgnh_status rc = entry(h, true); if (rc) return rc;
    const tgnh_context::PositionSnapshot& snap = h->snap;
    if (!snap.taken || !snap.d_posq) return fail(TGNH_ERR_STATE, "tgnh_restore_positions: no snapshot (tgnh_scale_positions with save != 0 takes one)");
    if (!snap.valid || snap.of_posq != h->bound.posq || snap.of_corr != h->bound.posq_corr)
        return fail(TGNH_ERR_STATE, "tgnh_restore_positions: the positions were rebound since the snapshot was taken");
    hipStream_t s = (hipStream_t)stream;
    Timed t(h, s, KID_OTHER);
    HIP_OK(hipMemcpyAsync(h->bound.posq, snap.d_posq, posq_bytes(h), hipMemcpyDeviceToDevice, s));
    if (corr_bytes(h)) HIP_OK(hipMemcpyAsync(h->bound.posq_corr, snap.d_corr, corr_bytes(h), hipMemcpyDeviceToDevice, s));
    return TGNH_OK;
}
