// tgnh_exchange.cpp -- the kinetic-energy sums across ranks: the mailbox exchange, RCCL bound at run time, the all-reduce hook; the resident share
#include <dlfcn.h>
#include <mutex>
// RCCL is bound with dlopen at run time (rccl() below); of its header only five types and three enumerators are used.  A ROCm
// install without the RCCL headers still builds this library (and the OpenMM glue): the declarations below are RCCL's ABI
// (rccl.h: ncclUniqueId is 128 bytes, ncclSuccess = 0, ncclSum = 0, ncclFloat64 = ncclDouble = 8).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
typedef enum { ncclDouble = 8 } ncclDataType_t;
}
#endif

#include "tgnh_host.h"

// ---------------------------------------------------------------------------
// mailbox exchange (SURVEY 8e done with stores over xGMI; protocol in tgnh_internal.h)
// ---------------------------------------------------------------------------
extern "C" tgnh_status tgnh_exchange_create(tgnh_handle h, int world, int rank, void* ipc_handle_out, void** mailbox_out) {
    CHECK_H(h);
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle");
    if (world < 1 || world > XCHG_MAX_WORLD || rank < 0 || rank >= world) return fail(TGNH_ERR_ARG, "bad world / rank");
    if (h->thermo.L.NT > MAX_GROUPS + 2) return fail(TGNH_ERR_UNSUPPORTED, "too many thermostats for a mailbox (more than 32 temperature groups: use an all-reduce hook or RCCL)");
    if (h->gather.chain) return fail(TGNH_ERR_UNSUPPORTED, "no mailbox for a chain too long for the LDS-resident form (it runs in gather_chain_kernel: use an all-reduce hook or RCCL)");
    if (h->xchg.mailbox) return fail(TGNH_ERR_STATE, "exchange already created");
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(h->xchg.mailbox.alloc(XCHG_MAILBOX_BYTES(world) / sizeof(unsigned long long), true, hipDeviceMallocUncached));
    HIP_OK(h->xchg.d_seq.alloc(1, true));
    HIP_OK(h->xchg.d_dead.alloc(1, true));
    HIP_OK(h->xchg.d_peers.alloc(world));
    HIP_OK(h->xchg.d_stat.alloc(3, true));
    HIP_OK(hipDeviceSynchronize());
    h->xchg.world = world; h->xchg.rank = rank;
    if (ipc_handle_out) {
        static_assert(sizeof(hipIpcMemHandle_t) == TGNH_XCHG_HANDLE_BYTES, "IPC handle size");
        hipIpcMemHandle_t ih;
        HIP_OK(hipIpcGetMemHandle(&ih, h->xchg.mailbox));
        std::memcpy(ipc_handle_out, &ih, sizeof(ih));
    }
    if (mailbox_out) *mailbox_out = h->xchg.mailbox;
    return TGNH_OK;
}

// the mailboxes carry the kinetic-energy sums only: a handle that removes its centre-of-mass motion inside the step loop
// (tgnh_set_cm_motion_removal) has no exchange for the momentum sums once they replace the hook; nor has one that rescales its
// velocities there (tgnh_set_velocity_rescaling) for the sums of a kinetic-energy pass outside the step's own
static tgnh_status cm_removal_off(tgnh_handle h, const char* what) {
    if (h->cmm.every > 0)
        return fail(TGNH_ERR_UNSUPPORTED, std::string(what) + ": centre-of-mass removal is on (tgnh_set_cm_motion_removal(h, 0) first)");
    if (h->resc.every > 0)
        return fail(TGNH_ERR_UNSUPPORTED, std::string(what) + ": velocity rescaling is on (tgnh_set_velocity_rescaling(h, 0, ...) first)");
    return TGNH_OK;
}

static tgnh_status exchange_finish_attach(tgnh_handle h, const std::vector<unsigned long long*>& peers) {
    HIP_OK(hipMemcpy(h->xchg.d_peers, peers.data(), sizeof(unsigned long long*) * peers.size(), hipMemcpyHostToDevice));
    h->xchg.args = XchgArgs{};
    h->xchg.args.on = 1; h->xchg.args.world = h->xchg.world; h->xchg.args.rank = h->xchg.rank;
    h->xchg.args.peers = h->xchg.d_peers; h->xchg.args.mine = h->xchg.mailbox; h->xchg.args.seq = h->xchg.d_seq; h->xchg.args.dead = h->xchg.d_dead;
    h->xchg.args.status = h->status.d_word;
    h->xchg.args.stat = h->xchg.d_stat;
    h->xchg.on = true;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_exchange_attach(tgnh_handle h, const void* ipc_handles) {
    CHECK_H(h);
    if (!h->xchg.mailbox) return fail(TGNH_ERR_STATE, "tgnh_exchange_create first");
    if (!ipc_handles) return fail(TGNH_ERR_ARG, "null handles");
    tgnh_status rc = cm_removal_off(h, "tgnh_exchange_attach"); if (rc) return rc;
    rc = deferred_guard(h, "tgnh_exchange_attach"); if (rc) return rc;
    h->owed.ke_carry = false;
    HIP_OK(hipSetDevice(h->device));
    std::vector<unsigned long long*> peers(h->xchg.world, nullptr);
    for (int r = 0; r < h->xchg.world; r++) {
        if (r == h->xchg.rank) { peers[r] = h->xchg.mailbox; continue; }
        hipIpcMemHandle_t ih;
        std::memcpy(&ih, static_cast<const char*>(ipc_handles) + (size_t)r * TGNH_XCHG_HANDLE_BYTES, sizeof(ih));
        void* p = nullptr;
        HIP_OK(hipIpcOpenMemHandle(&p, ih, hipIpcMemLazyEnablePeerAccess));
        h->xchg.opened.push_back(p);
        peers[r] = static_cast<unsigned long long*>(p);
    }
    return exchange_finish_attach(h, peers);
}

extern "C" tgnh_status tgnh_exchange_attach_pointers(tgnh_handle h, void* const* mailboxes) {
    CHECK_H(h);
    if (!h->xchg.mailbox) return fail(TGNH_ERR_STATE, "tgnh_exchange_create first");
    if (!mailboxes) return fail(TGNH_ERR_ARG, "null mailboxes");
    tgnh_status rc = cm_removal_off(h, "tgnh_exchange_attach_pointers"); if (rc) return rc;
    rc = deferred_guard(h, "tgnh_exchange_attach_pointers"); if (rc) return rc;
    h->owed.ke_carry = false;
    HIP_OK(hipSetDevice(h->device));
    std::vector<unsigned long long*> peers(h->xchg.world, nullptr);
    for (int r = 0; r < h->xchg.world; r++) {
        peers[r] = r == h->xchg.rank ? h->xchg.mailbox : static_cast<unsigned long long*>(mailboxes[r]);
        if (!peers[r]) return fail(TGNH_ERR_ARG, "null mailbox pointer");
    }
    return exchange_finish_attach(h, peers);
}

extern "C" tgnh_status tgnh_exchange_detach(tgnh_handle h) {
    CHECK_H(h);
    if (!h->xchg.on) return TGNH_OK;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipDeviceSynchronize());
    {   // a time-out that nobody has asked about yet
        uint32_t f = 0;
        HIP_OK(hipMemcpy(&f, h->status.d_word, sizeof(uint32_t), hipMemcpyDeviceToHost));
        note_status(h, f);
    }
    if (h->owed.end_pending && !h->status.failed_code) {          // settle collectively: every rank detaches at the same step
        tgnh_status rc = settle_end(h, (hipStream_t)0); if (rc) return rc;
        HIP_OK(hipDeviceSynchronize());
    }
    if (h->owed.chain_pending && h->owed.xwait_pending && !h->status.failed_code) {       // an exchange is half done (sent, not yet waited for): finish it
        tgnh_status rc = materialize_chain(h, (hipStream_t)0); if (rc) return rc;
        HIP_OK(hipDeviceSynchronize());
    }
    h->xchg.on = false;
    h->xchg.close_peers();                                  // (mine stays until tgnh_destroy)
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_allreduce(tgnh_handle h, tgnh_allreduce_fn fn, void* user) {
    CHECK_H(h);
    tgnh_status rc = deferred_guard(h, "tgnh_set_allreduce"); if (rc) return rc;
    h->owed.ke_carry = false;
    if (h->xchg.rccl_comm) { rc = tgnh_rccl_shutdown(h); if (rc) return rc; }
    h->xchg.allreduce = fn; h->xchg.allreduce_user = user;
    return TGNH_OK;
}

// ---------------------------------------------------------------------------
// RCCL: the all-reduce of SURVEY 8e enqueued by the library itself
// ---------------------------------------------------------------------------
// RCCL is bound at the first tgnh_rccl_* call, not at load time: the process may already hold one (PyTorch ships its own
// librccl.so.1 and a second copy in one address space is two sets of communicators), so the copy that is loaded is used, and
// the system's (/opt/rocm/lib) is opened only when there is none.  A library that never shards never touches RCCL.
namespace {
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
    bool ok = false;
};
void rccl_bind(Rccl& r);
Rccl& rccl() {                                   // (handles of different threads may reach this at once: bound exactly once)
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] { rccl_bind(r); });
    return r;
}
void rccl_bind(Rccl& r) {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) if (!r.lib) r.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);     // the copy the process already has
    for (const char* n : names) if (!r.lib) r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!r.lib) { r.error = std::string("RCCL not found (librccl.so.1): ") + dlerror(); return; }
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.lib, "ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce && r.GetErrorString;
    if (!r.ok) r.error = "RCCL: a required symbol is missing from librccl";
}
#define RCCL_OK(expr)                                                                                        \
    do {                                                                                                     \
        ncclResult_t r_ = (expr);                                                                            \
        if (r_ != ncclSuccess) return fail(TGNH_ERR_HIP, std::string(#expr) + ": " + rccl().GetErrorString(r_)); \
    } while (0)

// the tgnh_allreduce_fn the library installs for itself: the kinetic-energy sums, in place, on the step's stream
int rccl_allreduce(void* buf, int count, void* stream, void* user) {
    tgnh_context* h = static_cast<tgnh_context*>(user);
    return rccl().AllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, static_cast<ncclComm_t>(h->xchg.rccl_comm),
                            static_cast<hipStream_t>(stream)) == ncclSuccess ? 0 : 1;
}
}  // namespace

extern "C" tgnh_status tgnh_rccl_unique_id(void* id_out) {
    if (!id_out) return fail(TGNH_ERR_ARG, "null id");
    static_assert(sizeof(ncclUniqueId) == TGNH_RCCL_ID_BYTES, "ncclUniqueId size");
    if (!rccl().ok) return fail(TGNH_ERR_HIP, rccl().error);
    ncclUniqueId id;
    RCCL_OK(rccl().GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_rccl_comm(tgnh_handle h, void* nccl_comm) {
    CHECK_H(h);
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle");
    tgnh_status rc = deferred_guard(h, "tgnh_set_rccl_comm"); if (rc) return rc;
    h->owed.ke_carry = false;
    if (!rccl().ok) return fail(TGNH_ERR_HIP, rccl().error);
    if (h->xchg.rccl_comm) { rc = tgnh_rccl_shutdown(h); if (rc) return rc; }
    if (!nccl_comm) {                                   // (a hook the caller installed with tgnh_set_allreduce is not this call's to clear)
        if (h->xchg.allreduce == rccl_allreduce) { h->xchg.allreduce = nullptr; h->xchg.allreduce_user = nullptr; }
        return TGNH_OK;
    }
    h->xchg.rccl_comm = nccl_comm; h->xchg.rccl_owned = false;
    h->xchg.allreduce = rccl_allreduce; h->xchg.allreduce_user = h;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_rccl_init(tgnh_handle h, int world, int rank, const void* id) {
    CHECK_H(h);
    if (h->host_only) return fail(TGNH_ERR_STATE, "host-only handle");
    if (world < 1 || rank < 0 || rank >= world || !id) return fail(TGNH_ERR_ARG, "bad world / rank / id");
    tgnh_status rc = deferred_guard(h, "tgnh_rccl_init"); if (rc) return rc;
    h->owed.ke_carry = false;
    if (!rccl().ok) return fail(TGNH_ERR_HIP, rccl().error);
    if (h->xchg.rccl_comm) { rc = tgnh_rccl_shutdown(h); if (rc) return rc; }
    HIP_OK(hipSetDevice(h->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    RCCL_OK(rccl().CommInitRank(&comm, world, uid, rank));
    h->xchg.rccl_comm = comm; h->xchg.rccl_owned = true;
    h->xchg.allreduce = rccl_allreduce; h->xchg.allreduce_user = h;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_rccl_shutdown(tgnh_handle h) {
    CHECK_H(h);
    if (!h->xchg.rccl_comm) return TGNH_OK;
    if (!h->host_only) { HIP_OK(hipSetDevice(h->device)); HIP_OK(hipDeviceSynchronize()); }
    if (h->xchg.allreduce == rccl_allreduce) { h->xchg.allreduce = nullptr; h->xchg.allreduce_user = nullptr; }
    ncclComm_t comm = static_cast<ncclComm_t>(h->xchg.rccl_comm);
    const bool owned = h->xchg.rccl_owned;
    h->xchg.rccl_comm = nullptr; h->xchg.rccl_owned = false;
    if (owned) RCCL_OK(rccl().CommDestroy(comm));
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_get_resident_work_groups(tgnh_handle h, int* per_compute_unit) {
    CHECK_H(h);
    if (!per_compute_unit) return fail(TGNH_ERR_ARG, "null out");
    // of the kernel tgnh_get_resident_kernel names: with tgnh_set_resident_share and the compute units it says which grid steps
    // (wstep_kernel's count is the smaller of the two where a handle has both)
    int which = 0;
    tgnh_status rc = tgnh_get_resident_kernel(h, &which); if (rc) return rc;
    *per_compute_unit = which == 2 ? h->cfg.wresident_per_cu : which == 1 ? h->cfg.resident_per_cu : 0;
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_exchange_wait_stats(tgnh_handle h, void* stream, double* mean_us, double* max_us, int64_t* exchanges) {
    CHECK_H(h);
    if (!h->xchg.d_stat) return fail(TGNH_ERR_STATE, "tgnh_exchange_create first");
    HIP_OK(hipSetDevice(h->device));
    unsigned long long st[3] = {0, 0, 0};
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(st, h->xchg.d_stat, sizeof(st), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemsetAsync(h->xchg.d_stat, 0, sizeof(st), s));
    HIP_OK(hipStreamSynchronize(s));
    const double tick_us = 0.01;                           // wall_clock64: 100 MHz
    if (mean_us) *mean_us = st[2] ? tick_us * (double)st[0] / (double)st[2] : 0.0;
    if (max_us) *max_us = tick_us * (double)st[1];
    if (exchanges) *exchanges = (int64_t)st[2];
    return TGNH_OK;
}

extern "C" tgnh_status tgnh_set_resident_share(tgnh_handle h, int share) {
    CHECK_H(h);
    if (share < 1 || share > 64) return fail(TGNH_ERR_ARG, "resident share must be 1..64");
    h->cfg.resident_share = share;
    h->cfg.wresident_grid = 0;
    for (auto& g : h->cfg.resident_grid) g[0] = g[1] = 0;
    return TGNH_OK;
}
