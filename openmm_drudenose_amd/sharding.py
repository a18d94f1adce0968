"""Particle sharding over several contexts (include/drude_tgnh.h: tgnh_set_allreduce, tgnh_rccl_*, tgnh_exchange_*,
tgnh_set_resident_share): the all-reduce hook, the library's own RCCL all-reduce, the mailbox exchange over xGMI, and the share
of the device a one-launch step may fill."""
import ctypes as C
from types import SimpleNamespace

from . import _lib
from ._abi import _check
from .handle import Handle


class Sharding(Handle):
    def set_allreduce(self, fn):
        """fn(tensor_view) must sum the float64 device tensor in place over all ranks (stream-ordered)."""
        def _hook(buf, count, stream, user):
            try:
                t = self._ke_view(buf, count)
                fn(t)
                return 0
            except Exception as e:     # never unwind through C
                print("all-reduce hook failed:", e)
                return 1
        self._hook = _lib.ALLREDUCE_FN(_hook)
        self._views = {}
        _check(self.lib.tgnh_set_allreduce(self.h, self._hook, None))

    def _ke_view(self, ptr, count):
        key = (ptr, count)
        v = self._views.get(key)
        if v is None:
            hold = SimpleNamespace(__cuda_array_interface__={"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2})
            v = self.torch.as_tensor(hold, device=self.dev)
            self._views[key] = v
        return v

    # ---- the library's own RCCL all-reduce (include/drude_tgnh.h: tgnh_rccl_*) ----
    RCCL_ID_BYTES = 128

    def rccl_init(self, world, rank, unique_id):
        """Collective: every rank of `world` calls this with rank 0's id (rccl_unique_id())."""
        _check(self.lib.tgnh_rccl_init(self.h, int(world), int(rank), C.c_char_p(unique_id)))
        self._hook = None

    def rccl_unique_id(self):
        buf = C.create_string_buffer(self.RCCL_ID_BYTES)
        _check(self.lib.tgnh_rccl_unique_id(buf))
        return buf.raw

    def rccl_shutdown(self): _check(self.lib.tgnh_rccl_shutdown(self.h))

    def rccl_init_over(self, dist, rank, world):
        """The library's communicator set up through a torch.distributed process group (which only carries the 128-byte id):
        all ranks return True (the library enqueues ncclAllReduce itself from now on) or all return False (nothing changed)."""
        ok, err = 1, None
        ids = [None]
        # ncclCommInitRank is collective: a rank that cannot even bind RCCL must say so BEFORE anybody enters it, or its peers
        # wait inside it for good.  Every rank therefore makes an id of its own first (binds the library, not collective) and
        # the ranks vote; only rank 0's id is used.
        try:
            mine = self.rccl_unique_id()
            if rank == 0:
                ids[0] = mine
        except Exception as e:                      # noqa: BLE001
            ok, err = 0, e
        votes = [None] * world
        dist.all_gather_object(votes, ok)
        if not all(votes):
            self.rccl_error = err or RuntimeError("RCCL could not be bound on rank(s) " + str([r for r, v in enumerate(votes) if not v]))
            return False
        dist.broadcast_object_list(ids, src=0)
        try:
            self.rccl_init(world, rank, ids[0])
        except Exception as e:                      # noqa: BLE001
            ok, err = 0, e
        flags = [None] * world
        dist.all_gather_object(flags, ok)
        if not all(flags):
            if ok:
                self.rccl_shutdown()
            self.rccl_error = err
            return False
        return True

    # ---- mailbox exchange over xGMI (include/drude_tgnh.h: tgnh_exchange_*) ----
    XCHG_HANDLE_BYTES = 64

    def exchange_wait_stats(self):
        """(mean us, max us, exchanges) of this rank's waits for its peers' sums since the last call; resets."""
        return self._get(self.lib.tgnh_exchange_wait_stats, (C.c_double, C.c_double, C.c_int64), stream=True)

    def exchange_create(self, world, rank):
        """-> (IPC handle bytes for peers in other processes, device pointer for peers in this process)"""
        buf = C.create_string_buffer(self.XCHG_HANDLE_BYTES)
        ptr = self._get(self.lib.tgnh_exchange_create, C.c_void_p, int(world), int(rank), buf)
        return buf.raw, ptr

    def exchange_attach(self, handles):
        """handles: every rank's IPC handle bytes, in rank order (own entry ignored)."""
        _check(self.lib.tgnh_exchange_attach(self.h, b"".join(handles)))

    def exchange_attach_pointers(self, pointers):
        arr = (C.c_void_p * len(pointers))(*[C.c_void_p(p) for p in pointers])
        _check(self.lib.tgnh_exchange_attach_pointers(self.h, arr))

    def exchange_detach(self): _check(self.lib.tgnh_exchange_detach(self.h))

    def attach_exchange_over(self, dist, rank, world, tensor_device="cuda"):
        """Collective over a torch.distributed process group: every rank creates its mailbox, the hipIpc handles go
        round with all_gather_object, every rank maps its peers.  All ranks return the same answer: True = the
        mailbox exchange is attached everywhere; False = nowhere (a rank could not create / map: the all-reduce hook,
        if set, keeps doing the exchange)."""
        ok, err = 1, None
        try:
            handle, _ = self.exchange_create(world, rank)
            handles = [None] * world
            dist.all_gather_object(handles, handle)
            self.exchange_attach(handles)
        except Exception as e:                      # noqa: BLE001 -- any failure means "not here", decided collectively below
            ok, err = 0, e
        t = self.torch.tensor([ok], dtype=self.torch.int32, device=tensor_device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if int(t.item()) == 0:
            if ok:
                self.exchange_detach()
            self.exchange_error = err
            return False
        return True

    # ---- the one-launch step's share of the device (FLAG_RESIDENT_STEP) ----
    def set_resident_share(self, share):
        """FLAG_RESIDENT_STEP: this context may fill 1/share of the device (several contexts stepping concurrently)."""
        _check(self.lib.tgnh_set_resident_share(self.h, int(share)))

    def resident_work_groups(self):
        """Work-groups per compute unit found resident together at create, of the kernel resident_kernel() names (0: the deferred
        launches run)."""
        return self._get(self.lib.tgnh_get_resident_work_groups)

    def resident_kernel(self):
        """The kernel the next step_begin runs as its one launch: None, 'step_kernel' or 'wstep_kernel'."""
        return (None, "step_kernel", "wstep_kernel")[self._get(self.lib.tgnh_get_resident_kernel)]
