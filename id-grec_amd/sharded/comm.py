"""`comm` of the sharded step: torch.distributed, libidgrec's own RCCL communicator, the choice between them, and the
world-1 stub (the interface: __init__.py)."""
import os

import numpy as np


class TorchComm:
    """`comm` on torch.distributed (backend "nccl" == RCCL over xGMI on ROCm).  With the gloo
    backend (tests: two ranks sharing one GPU, or CPU arrays) device tensors are staged through
    the host."""

    def __init__(self, dist):
        self.dist = dist
        self.backend = dist.get_backend()
        self.world, self.rank = dist.get_world_size(), dist.get_rank()
        # The sharded step issues 8 collectives; dist.all_reduce() spends ~25 us of host time per call in argument
        # checks before it reaches the process group.  Call the group object directly when this torch exposes it.
        self._pg = self._opts = self._opts_avg = None
        self.averages = self.backend == "nccl"  # RCCL divides inside the collective (ReduceOp.AVG); gloo cannot
        try:
            self._pg = dist.distributed_c10d._get_default_group()
            self._opts = dist.AllreduceOptions()
            self._opts.reduceOp = dist.ReduceOp.SUM
            self._opts_avg = dist.AllreduceOptions()
            self._opts_avg.reduceOp = dist.ReduceOp.AVG
        except Exception:  # noqa: BLE001 - private API: fall back to the public wrapper
            self._pg = None

    def all_reduce_async(self, t, average=False):
        """Sum over ranks; average=True asks for the mean and gets it only when self.averages (otherwise the sum —
        the caller scales)."""
        import torch

        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)  # shares memory
        if self.backend == "gloo" and t.is_cuda:
            host = t.cpu()
            self.dist.all_reduce(host)
            t.copy_(host)
            return None
        avg = average and self.averages
        if self._pg is not None and t.is_cuda:
            return self._pg.allreduce([t], self._opts_avg if avg else self._opts)
        return self.dist.all_reduce(t, op=self.dist.ReduceOp.AVG if avg else self.dist.ReduceOp.SUM, async_op=True)

    def all_gather_async(self, out, t):
        """out (world x len(t) elements, rank-major) <- every rank's t; t may be this rank's block of out (in place)."""
        import torch

        if isinstance(t, np.ndarray):
            t, out = torch.from_numpy(t), torch.from_numpy(out)  # share memory
        if self.backend == "gloo":
            # (the rehearsal backend: staged through a host copy, which also makes the in-place form safe)
            host = torch.empty(out.shape, dtype=out.dtype)
            self.dist.all_gather_into_tensor(host, t.cpu().contiguous())
            out.copy_(host)
            return None
        return self.dist.all_gather_into_tensor(out, t, async_op=True)

    def reduce_scatter_async(self, t):
        """t = world equal blocks; this rank's block <- the sum over ranks of that block, in place (the other blocks are
        left in an unspecified state).  gloo has no reduce-scatter: the rehearsal backend all-reduces the whole buffer."""
        import torch

        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        if self.backend == "gloo":
            return self.all_reduce_async(t)
        flat = t.view(-1)
        c = flat.numel() // self.world
        own = flat[self.rank * c:(self.rank + 1) * c]
        out = torch.empty_like(own)  # (c10d does not promise the in-place form: reduce into a scratch block, then copy)
        work = self.dist.reduce_scatter_tensor(out, flat, async_op=True)
        return ("copy_after", work, own, out)

    def all_to_all_async(self, recv, send):
        """Block p of `send` (world equal blocks) goes to rank p; block p of `recv` receives rank p's block for this rank."""
        import torch

        if isinstance(send, np.ndarray):
            send, recv = torch.from_numpy(send), torch.from_numpy(recv)
        if self.backend == "gloo":
            # (the rehearsal backend has no all-to-all: point-to-point pairs on host copies, completed inside the call)
            s, r = send.detach().cpu().view(self.world, -1), torch.empty(recv.shape, dtype=recv.dtype).view(self.world, -1)
            r[self.rank] = s[self.rank]
            reqs = []
            for p in range(self.world):
                if p != self.rank:
                    reqs.append(self.dist.isend(s[p].contiguous(), p))
                    reqs.append(self.dist.irecv(r[p], p))
            for q in reqs:
                q.wait()
            recv.view(self.world, -1).copy_(r)
            return None
        return self.dist.all_to_all_single(recv.view(-1), send.view(-1), async_op=True)

    def wait(self, work):
        if isinstance(work, tuple):  # reduce_scatter_async: the reduced block goes to its place once the collective is done
            _, inner, own, out = work
            inner.wait()
            own.copy_(out)
        elif work is not None:
            work.wait()


class NativeComm:
    """`comm` on libidgrec's own RCCL communicator (idg_comm_*, include/idgrec.h): collectives are enqueued on the
    CURRENT HIP stream, in order with the kernels around them — no second stream, no event pair and no work object
    per call (torch.distributed's process group costs ~20 us of host time and two cross-stream waits per
    collective, which is most of a step on the small graphs).  torch.distributed is used once, to hand rank 0's
    unique id to the other ranks."""

    averages = True
    _generation = 0

    def __init__(self, dist, device_index, overlap_bytes=64 << 20):
        """overlap_bytes: collectives of at least this many bytes run on a stream of their own, ordered after the
        current stream by an event, so that the caller's next kernels overlap them until wait(); smaller ones stay on
        the current stream (the two cross-stream waits cost ~40 us of host time per collective — measured on the
        9.7 MB item panel of the yelp2018 shape: 0.69 ms per sharded step with them, 0.53 without)."""
        import ctypes as C

        import torch

        from .. import native

        self.torch, self.lib, self.check = torch, native.lib, native.check
        self.world = dist.get_world_size()
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")  # the copy this process already runs
        self.check(self.lib.idg_comm_load(path.encode() if os.path.exists(path) else None), "idg_comm_load")
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        uid = torch.zeros(128, dtype=torch.uint8)
        NativeComm._generation += 1
        key = "idg_comm_unique_id_%d" % NativeComm._generation  # every rank constructs communicators in the same order
        failure = None
        if self.rank == 0:
            try:
                self.check(self.lib.idg_comm_unique_id(uid.data_ptr()), "idg_comm_unique_id")
            except Exception as exc:  # noqa: BLE001 - the other ranks must learn of it instead of waiting for an id
                failure = exc
        if self.world > 1:
            # through the rendezvous store, not a collective (torch's own RCCL communicator and its streams are then
            # created after this one's; see ops.side_stream for what stream order does to hardware-queue placement)
            store = dist.distributed_c10d._get_default_store()
            if self.rank == 0:
                store.set(key, b"FAILED" if failure is not None else bytes(uid.numpy().tobytes()))
            got = bytes(store.get(key))
            if got == b"FAILED" and failure is None:
                failure = RuntimeError("rank 0 could not obtain an RCCL unique id")
            if failure is None:
                uid = torch.frombuffer(bytearray(got), dtype=torch.uint8).clone()
        if self.world > 1:
            # idg_comm_create is collective (ncclCommInitRank): a rank that cannot take part — no id, or a device
            # index this process cannot open — must say so BEFORE the others enter it, or they wait there for good.
            # Every rank publishes a verdict under this communicator's generation and reads everyone else's.
            ready = failure is None and 0 <= int(device_index) < torch.cuda.device_count()
            store.set("idg_comm_ready_%d_%d" % (NativeComm._generation, self.rank), b"1" if ready else b"0")
            bad = [r for r in range(self.world)
                   if bytes(store.get("idg_comm_ready_%d_%d" % (NativeComm._generation, r))) != b"1"]
            if bad and failure is None:
                failure = RuntimeError("libidgrec communicator: rank(s) %s cannot join (no unique id or no such device)" % bad)
        if failure is not None:
            raise failure
        handle = C.c_void_p()
        self.check(self.lib.idg_comm_create(self.rank, self.world, uid.data_ptr(), int(device_index), C.byref(handle)),
                   "idg_comm_create")
        self.handle = handle
        self._force = False  # self_test(): enqueue on RCCL even at world size 1, where a collective is the identity
        self.overlap_bytes = int(overlap_bytes)
        self._own = self._own_raw = None   # the collectives' own stream, made on first use
        self._ring, self._next = [], 0     # (issued, done) event pairs, reused round-robin (a step issues up to 4 x slices collectives here; a handle is waited for within the next step)

    def _fork(self):
        """Order the communicator's stream after the current one; returns (raw stream handle, event to record when done)."""
        torch = self.torch
        if self._own is None:
            self._own = torch.cuda.Stream()
            self._own_raw = self._own.cuda_stream
            self._ring = [(torch.cuda.Event(), torch.cuda.Event()) for _ in range(128)]  # > 3 steps' worth of collectives
        issued, done = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        issued.record()
        self._own.wait_event(issued)
        return self._own_raw, done

    @staticmethod
    def _stream():
        from ..ops import _stream

        return _stream()

    def _f32(self, t):
        assert t.is_cuda and t.dtype == self.torch.float32 and t.is_contiguous(), "NativeComm moves contiguous fp32 device tensors"
        return t.data_ptr()

    def timed_stream(self, nbytes):
        """The torch stream a collective of nbytes will run on when it is NOT the current one (TimelineComm), else None."""
        if (self.world == 1 and not self._force) or nbytes < self.overlap_bytes:
            return None
        if self._own is None:
            self._fork()  # creates the stream (the ring slot it takes is harmless)
        return self._own

    def all_reduce_async(self, t, average=False):
        if self.world == 1 and not self._force:  # (the identity: nothing to enqueue; self_test() still runs RCCL itself)
            return None
        if t.numel() * 4 >= self.overlap_bytes:
            stream, done = self._fork()
            self.check(self.lib.idg_allreduce_f32(self.handle, self._f32(t), t.numel(), int(bool(average)), stream),
                       "idg_allreduce_f32")
            done.record(self._own)
            return done
        self.check(self.lib.idg_allreduce_f32(self.handle, self._f32(t), t.numel(), int(bool(average)), self._stream()),
                   "idg_allreduce_f32")
        return None

    def all_gather_async(self, out, t):
        assert out.numel() == t.numel() * self.world
        if self.world == 1 and not self._force:
            if out.data_ptr() != t.data_ptr():
                out.view(-1).copy_(t.view(-1))
            return None
        if out.numel() * 4 >= self.overlap_bytes:
            stream, done = self._fork()
            self.check(self.lib.idg_allgather_f32(self.handle, self._f32(t), self._f32(out), t.numel(), stream),
                       "idg_allgather_f32")
            done.record(self._own)
            return done
        self.check(self.lib.idg_allgather_f32(self.handle, self._f32(t), self._f32(out), t.numel(), self._stream()),
                   "idg_allgather_f32")
        return None

    def reduce_scatter_async(self, t):
        """t = world equal blocks; this rank's block <- the sum over ranks of that block, in place."""
        c = t.numel() // self.world
        assert c * self.world == t.numel(), "reduce-scatter of %d floats over %d ranks" % (t.numel(), self.world)
        if self.world == 1 and not self._force:
            return None
        base = self._f32(t)
        own = base + 4 * c * self.rank
        if t.numel() * 4 >= self.overlap_bytes:
            stream, done = self._fork()
            self.check(self.lib.idg_reduce_scatter_f32(self.handle, base, own, c, stream), "idg_reduce_scatter_f32")
            done.record(self._own)
            return done
        self.check(self.lib.idg_reduce_scatter_f32(self.handle, base, own, c, self._stream()), "idg_reduce_scatter_f32")
        return None

    def all_to_all_async(self, recv, send):
        """Block p of `send` goes to rank p; block p of `recv` receives rank p's block for this rank (idg_alltoall_f32:
        grouped ncclSend / ncclRecv)."""
        c = send.numel() // self.world
        assert c * self.world == send.numel() == recv.numel(), "all-to-all of %d floats over %d ranks" % (send.numel(), self.world)
        flags = 1 if self._force else 0  # (tests at world size 1: the own block through ncclSend / ncclRecv too)
        if send.numel() * 4 >= self.overlap_bytes and not (self.world == 1 and not self._force):
            stream, done = self._fork()
            self.check(self.lib.idg_alltoall_f32(self.handle, self._f32(send), self._f32(recv), c, flags, stream), "idg_alltoall_f32")
            done.record(self._own)
            return done
        self.check(self.lib.idg_alltoall_f32(self.handle, self._f32(send), self._f32(recv), c, flags, self._stream()),
                   "idg_alltoall_f32")
        return None

    def wait(self, work):
        if work is not None:
            self.torch.cuda.current_stream().wait_event(work)

    def through_rccl(self):
        """Context manager: at world size 1 a collective is the identity and is normally not enqueued at all; inside this
        context it goes through RCCL as on a larger world (tests, the self-test)."""
        import contextlib

        @contextlib.contextmanager
        def forced():
            old, self._force = self._force, True
            try:
                yield self
            finally:
                self._force = old

        return forced()

    def self_test(self):
        """All-reduce (both stream routes), all-gather and reduce-scatter + in-place all-gather with known answers; True when
        all are right on this rank.  Runs through RCCL at any world size."""
        with self.through_rccl():
            return self._self_test()

    def _self_test(self):
        torch = self.torch
        a = torch.full((1024,), float(self.rank + 1), dtype=torch.float32, device="cuda")
        g = torch.zeros(1024 * self.world, dtype=torch.float32, device="cuda")
        self.all_gather_async(g, a)
        self.all_reduce_async(a)
        big = torch.full((self.overlap_bytes // 4 + 1024,), float(self.rank + 1), dtype=torch.float32, device="cuda")
        work = self.all_reduce_async(big, average=True)   # the second-stream form
        self.wait(work)
        big += 1.0                                        # ordered after the collective by wait()
        # reduce-scatter + in-place all-gather of the reduced blocks == all-reduce (what ends a sharded step)
        rs = (torch.arange(1024 * self.world, dtype=torch.float32, device="cuda") % 7) * float(self.rank + 1)
        rs_want = (torch.arange(1024 * self.world, dtype=torch.float32, device="cuda") % 7) * (self.world * (self.world + 1) / 2)
        self.wait(self.reduce_scatter_async(rs))
        self.wait(self.all_gather_async(rs, rs[1024 * self.rank: 1024 * (self.rank + 1)]))
        torch.cuda.synchronize()
        want = torch.arange(1, self.world + 1, dtype=torch.float32, device="cuda").repeat_interleave(1024)
        return (bool((a == self.world * (self.world + 1) / 2).all().item()) and bool(torch.equal(g, want))
                and bool((big == (self.world + 1) / 2 + 1.0).all().item()) and bool(torch.equal(rs, rs_want)))

    def close(self):
        if self.handle is not None:
            self.torch.cuda.synchronize()
            self.lib.idg_comm_destroy(self.handle)
            self.handle = None


def make_comm(dist, kind="auto"):
    """kind: "torch" (torch.distributed process group), "native" (libidgrec's RCCL communicator; fails loudly if it
    cannot be set up) or "auto": native when the backend is nccl and EVERY rank both set it up and passed its
    self-test, torch.distributed otherwise (both are RCCL over xGMI; the choice is recorded in the bench line)."""
    import torch

    if kind == "torch" or (kind == "auto" and dist.get_backend() != "nccl"):
        return TorchComm(dist), "torch.distributed"
    if kind == "native":
        comm = NativeComm(dist, torch.cuda.current_device())
        assert comm.self_test(), "libidgrec RCCL communicator: self-test failed"
        return comm, "libidgrec RCCL communicator"
    # auto: agree rank by rank before the collective idg_comm_create (a rank that cannot load the library must not
    # leave the others waiting inside ncclCommInitRank)
    from .. import native

    path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    loaded = native.lib.idg_comm_load(path.encode() if os.path.exists(path) else None) == 0
    rank, world = dist.get_rank(), dist.get_world_size()
    try:
        store = dist.distributed_c10d._get_default_store()  # no collective yet: see NativeComm.__init__
    except Exception:  # noqa: BLE001 - private torch API: without it there is no collective-free way to agree
        return TorchComm(dist), "torch.distributed (rendezvous store not reachable)"
    # keys carry the generation of the communicator about to be built (every rank calls make_comm in the same order),
    # so a second make_comm on the same process group never reads the first one's verdicts
    gen = NativeComm._generation + 1
    store.set("idg_comm_loaded_%d_%d" % (gen, rank), b"1" if loaded else b"0")
    if not all(bytes(store.get("idg_comm_loaded_%d_%d" % (gen, r))) == b"1" for r in range(world)):
        return TorchComm(dist), "torch.distributed (libidgrec could not load librccl)"
    why = ""
    try:
        comm = NativeComm(dist, torch.cuda.current_device())
        good = comm.self_test()
    except Exception as exc:  # noqa: BLE001 - any failure selects the other RCCL path, and is reported
        comm, good = None, False
        why = str(exc)[:120]
    ok = torch.tensor([1 if good else 0], dtype=torch.int32, device="cuda")
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 1:
        return comm, "libidgrec RCCL communicator"
    return TorchComm(dist), "torch.distributed (libidgrec communicator unavailable%s)" % ((": " + why) if comm is None else "")


class NoComm:
    """world_size 1."""

    averages = True
    world = 1
    rank = 0

    def all_reduce_async(self, t, average=False):
        return None

    def all_gather_async(self, out, t):
        same = (out.data_ptr() == t.data_ptr()) if hasattr(out, "data_ptr") else np.shares_memory(out, t)
        if not same:  # (in place at world size 1: nothing moves)
            out[...] = t
        return None

    def reduce_scatter_async(self, t):
        return None

    def all_to_all_async(self, recv, send):
        recv[...] = send
        return None

    def wait(self, work):
        pass
