// tgnh_frames.cpp -- the periodic box (tgnh_set_periodic_box, tgnh_get_periodic_box), tgnh_wrap_molecules, and the compact frame
// (tgnh_get_frame_count, tgnh_write_frame): the molecule table's second user (tgnh_positions.cpp builds it; tgnh_wrap.hip has the kernels)
#include "tgnh_host.h"
#include "tgnh_wrap.h"

// ---------------------------------------------------------------------------
// the box (include/drude_tgnh.h has the contract): host side only, handed to every launch by value
// ---------------------------------------------------------------------------
extern "C" tgnh_status tgnh_set_periodic_box(tgnh_handle h, const double a[3], const double b[3], const double c[3]) {
    CHECK_H(h);
    if (!a || !b || !c) return fail(TGNH_ERR_ARG, "tgnh_set_periodic_box: a null box vector");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(a[k]) || !std::isfinite(b[k]) || !std::isfinite(c[k])) return fail(TGNH_ERR_ARG, "tgnh_set_periodic_box: a component is not finite");
    if (a[1] != 0.0 || a[2] != 0.0 || b[2] != 0.0)
        return fail(TGNH_ERR_ARG, "tgnh_set_periodic_box: not in reduced form: a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz)");
    if (!(a[0] > 0.0) || !(b[1] > 0.0) || !(c[2] > 0.0)) return fail(TGNH_ERR_ARG, "tgnh_set_periodic_box: ax, by and cz must be positive");
    if (!(a[0] >= 2.0 * std::fabs(b[0])) || !(a[0] >= 2.0 * std::fabs(c[0])) || !(b[1] >= 2.0 * std::fabs(c[1])))
        return fail(TGNH_ERR_ARG, "tgnh_set_periodic_box: not in reduced form: ax >= 2 |bx|, ax >= 2 |cx| and by >= 2 |cy| are required");
    tgnh_context::PeriodicBox& box = h->box;
    std::memcpy(box.a, a, sizeof box.a); std::memcpy(box.b, b, sizeof box.b); std::memcpy(box.c, c, sizeof box.c);
    box.set = true;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_periodic_box(tgnh_handle h, double a[3], double b[3], double c[3]) {
    CHECK_H(h);
    if (!a || !b || !c) return fail(TGNH_ERR_ARG, "tgnh_get_periodic_box: a null box vector");
    const tgnh_context::PeriodicBox& box = h->box;
    if (!box.set) return fail(TGNH_ERR_STATE, "tgnh_get_periodic_box: no periodic box has been set (tgnh_set_periodic_box)");
    std::memcpy(a, box.a, sizeof box.a); std::memcpy(b, box.b, sizeof box.b); std::memcpy(c, box.c, sizeof box.c);
    return TGNH_OK;
}

static void box_args(const tgnh_context* c, WrapArgs& a) {
    const tgnh_context::PeriodicBox& box = c->box;
    a.box[0] = box.a[0]; a.box[1] = box.b[0]; a.box[2] = box.b[1]; a.box[3] = box.c[0]; a.box[4] = box.c[1]; a.box[5] = box.c[2];
}

// the molecule table's part of the launch arguments, after molecules_device and molecules_launch_bounds
static void table_args(const tgnh_context* c, WrapArgs& a) {
    const tgnh_context::Molecules& m = c->mol;
    a.posq = c->bound.posq; a.corr = c->bound.posq_corr; a.n = c->d.num_particles;
    a.num_molecules = m.t.count;
    if (m.t.spans) {
        a.span_first = m.d_span_first; a.span_heads = m.d_span_heads; a.num_spans = (int)m.t.span_heads.size();
        a.span_out = m.d_span_out; a.span_drude = m.d_span_drude;
    } else {
        a.mol_of = m.d_mol_of; a.mem_start = m.d_mem_start; a.members = m.d_members; a.shift = m.d_shift;
    }
}

// ---------------------------------------------------------------------------
// tgnh_wrap_molecules
// ---------------------------------------------------------------------------
extern "C" tgnh_status tgnh_wrap_molecules(tgnh_handle h, void* stream) {
    CHECK_H(h);
    if (!h->box.set) return fail(TGNH_ERR_STATE, "tgnh_wrap_molecules: no periodic box has been set (tgnh_set_periodic_box)");
    tgnh_status rc = entry(h, true); if (rc) return rc;           // (buffers bound, not a host-only handle, no failure seen before)
    hipStream_t s = (hipStream_t)stream;
    rc = molecules_ensure(h, "tgnh_wrap_molecules"); if (rc) return rc;
    // (a half kick owed to velm does not stand in the way: the forces of a periodic system are those of the moved molecules too)
    rc = molecules_device(h, s); if (rc) return rc;
    rc = molecules_launch_bounds(h); if (rc) return rc;
    WrapArgs a{};
    table_args(h, a);
    box_args(h, a);
    Timed t(h, s, KID_OTHER);
    if (h->mol.t.spans) HIP_OK(launch_wrap_spans(h->d.precision, a, s));
    else HIP_OK(launch_wrap_table(h->d.precision, a, s));
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// the frame
// ---------------------------------------------------------------------------
enum { FRAME_FLAGS = TGNH_FRAME_WRAP | TGNH_FRAME_SKIP_DRUDE | TGNH_FRAME_INTERLEAVED };

// output indices by slot: i minus the Drude slots below i, -1 for a Drude slot (host side; needs no device)
static void frame_index(tgnh_context* c) {
    tgnh_context::Frames& f = c->frames;
    if (f.kept >= 0) return;
    const int N = c->d.num_particles;
    f.out_index.assign((size_t)N, 0);
    for (int d : c->topo.pair_drude) f.out_index[d] = -1;
    int kept = 0;
    for (int i = 0; i < N; i++)
        if (f.out_index[i] == 0) f.out_index[i] = kept++;
    f.kept = kept;
}

static int64_t frame_count(tgnh_context* c, int flags) {
    if (!(flags & TGNH_FRAME_SKIP_DRUDE)) return c->d.num_particles;
    frame_index(c);
    return c->frames.kept;
}

extern "C" tgnh_status tgnh_get_frame_count(tgnh_handle h, int32_t flags, int64_t* count) {
    CHECK_H(h);
    if (!count) return fail(TGNH_ERR_ARG, "tgnh_get_frame_count: null count");
    if (flags & ~FRAME_FLAGS) return fail(TGNH_ERR_ARG, "tgnh_get_frame_count: an unknown flag");
    *count = frame_count(h, flags);
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_write_frame(tgnh_handle h, const tgnh_frame_desc* desc, float* out, void* stream) {
    CHECK_H(h);
    if (!desc || !out) return fail(TGNH_ERR_ARG, "tgnh_write_frame: null desc or out");
    if (desc->struct_size != sizeof(tgnh_frame_desc)) return fail(TGNH_ERR_ARG, "tgnh_write_frame: desc->struct_size is not sizeof(tgnh_frame_desc)");
    const int flags = desc->flags;
    if (flags & ~FRAME_FLAGS) return fail(TGNH_ERR_ARG, "tgnh_write_frame: an unknown flag");
    if (!std::isfinite(desc->unit) || !(desc->unit > 0.0)) return fail(TGNH_ERR_ARG, "tgnh_write_frame: unit is not finite or not positive");
    const int64_t count = frame_count(h, flags);
    const bool inter = (flags & TGNH_FRAME_INTERLEAVED) != 0;
    if (inter ? desc->stride != 0 : desc->stride < count)
        return fail(TGNH_ERR_ARG, inter ? "tgnh_write_frame: stride must be 0 in the interleaved layout" : "tgnh_write_frame: stride is smaller than the frame's count");
    const int64_t need = inter ? 3 * count : 2 * desc->stride + count;
    if (desc->capacity < need)
        return fail(TGNH_ERR_ARG, "tgnh_write_frame: capacity is " + std::to_string(desc->capacity) + " floats, the frame takes " + std::to_string(need));
    const bool wrap = (flags & TGNH_FRAME_WRAP) != 0, skip = (flags & TGNH_FRAME_SKIP_DRUDE) != 0;
    if (wrap && !h->box.set) return fail(TGNH_ERR_STATE, "tgnh_write_frame: TGNH_FRAME_WRAP without a periodic box (tgnh_set_periodic_box)");
    tgnh_status rc = entry(h, true); if (rc) return rc;           // (buffers bound, not a host-only handle, no failure seen before)
    hipStream_t s = (hipStream_t)stream;
    const bool cap = stream_capturing(s);
    if (!cap) {                                                   // where the runtime knows the allocation behind out, it must hold `capacity` floats
        hipDeviceptr_t base = nullptr; size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, out) != hipSuccess) (void)hipGetLastError();      // (mapped by other means: the caller's word is taken)
        else {
            const size_t left = size - (size_t)(reinterpret_cast<const char*>(out) - static_cast<const char*>(base));
            if (left / sizeof(float) < (size_t)desc->capacity)
                return fail(TGNH_ERR_ARG, "tgnh_write_frame: out has " + std::to_string(left) + " bytes behind the pointer, capacity says " +
                                              std::to_string(desc->capacity) + " floats");
        }
    }
    if (wrap) {
        rc = molecules_ensure(h, "tgnh_write_frame"); if (rc) return rc;
        rc = molecules_device(h, s); if (rc) return rc;
        rc = molecules_launch_bounds(h); if (rc) return rc;
    }
    if (h->d.precision == TGNH_PREC_MIXED && !h->bound.posq_corr) return fail(TGNH_ERR_STATE, "internal: mixed precision without a position correction");
    const bool by_index = skip && !(wrap && h->mol.t.spans);     // the launches that find j in out_index
    tgnh_context::Frames& f = h->frames;
    if (by_index && !f.d_out_index) {
        if (cap) return fail(TGNH_ERR_STATE, "tgnh_write_frame: the table of output indices is not on the device yet and the stream is capturing "
                                             "(call tgnh_write_frame once with these flags outside the capture)");
        frame_index(h);
        if ((int)f.out_index.size() != h->d.num_particles) return fail(TGNH_ERR_STATE, "internal: the output indices do not cover the slots");
        HIP_OK(f.d_out_index.upload(f.out_index));
    }
    WrapArgs a{};
    a.posq = h->bound.posq; a.corr = h->bound.posq_corr; a.n = h->d.num_particles;
    if (wrap) { table_args(h, a); box_args(h, a); }
    a.out = out; a.count = count; a.unit = desc->unit; a.skip_drude = skip;
    a.plane = inter ? 1 : desc->stride; a.step = inter ? 3 : 1;
    if (by_index) a.out_index = f.d_out_index;
    Timed t(h, s, KID_OTHER);
    if (!wrap) HIP_OK(launch_frame_plain(h->d.precision, a, s));
    else if (h->mol.t.spans) HIP_OK(launch_frame_spans(h->d.precision, a, s));
    else HIP_OK(launch_frame_table(h->d.precision, a, s));
    return TGNH_OK;
}
