"""`kernels` of the sharded step bound to libidgrec.so (the interface: __init__.py)."""
import numpy as np


# --------------------------------------------------------------------------- product bindings
class HipKernels:
    """`kernels` bound to libidgrec.so on the current HIP device.  The step issues ~40 library calls; what is marshalled
    here is kept minimal (the engine hands over the same preallocated buffers every step: pointers and views are cached,
    arguments are not re-validated — the wrappers in ops/ do that for everybody else)."""

    def __init__(self, device=None):
        import ctypes as C

        import torch

        from .. import native, ops

        self.torch, self.ops, self.C = torch, ops, C
        self.lib, self.check, self.Epilogue, self.ShardPrep = native.lib, native.check, native.Epilogue, native.ShardPrep
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._pool = []
        self._bits = {}
        self._ws = {}
        # side stream of the batch preparation, claimed at construction (ops.side_stream: hardware-queue placement)
        self._side = ops.side_stream(self.device)
        self._side_raw = self._side.cuda_stream
        self._fork = ops.LocalEvent()

    def zeros(self, shape):
        return self.torch.zeros(shape, dtype=self.torch.float32, device=self.device)

    def fill(self, a, v):
        a.fill_(v)

    def make_graph(self, indptr, indices, values, n_rows, n_cols):
        # both orientations (R_g and R_g^T) are built explicitly by shard_adjacency
        return self.ops.Graph(indptr, indices, values, n_rows, n_cols, device=self.device, symmetric=False,
                              build_transpose=False)

    def spmm(self, graph, X, Y=None, addend=None, sums=(), sum_out=None, div=1.0, accumulate=False, mask=None, adam=None,
             out_rows=None, x_rows=None, discard_grad=False, Y24=None):
        """idg_spmm_epi_f32 (include/idgrec.h): the product with the whole epilogue.  Y24: the finished rows as 24-bit values
        (a packed exchange's send buffer) instead of / beside Y."""
        d = X.shape[1]
        n_s = len(sums)
        e = self.Epilogue(None if Y is None else Y.data_ptr(), None if addend is None else addend.data_ptr(),
                          sums[0].data_ptr() if n_s > 0 else None, sums[1].data_ptr() if n_s > 1 else None,
                          sums[2].data_ptr() if n_s > 2 else None, None if sum_out is None else sum_out.data_ptr(), d, div,
                          1 if accumulate else 0, None if mask is None else mask.data_ptr())
        if adam is not None:
            p, m, v, lr, step = adam
            e.adam_param, e.adam_exp_avg, e.adam_exp_avg_sq = p.data_ptr(), m.data_ptr(), v.data_ptr()
            e.adam_lr, e.adam_beta1, e.adam_beta2, e.adam_eps, e.adam_step = lr, 0.9, 0.999, 1e-8, step
            e.adam_discard_grad = 1 if discard_grad else 0
        if Y24 is not None:
            e.y24 = Y24.data_ptr()
        key = (id(graph), d)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = (graph, graph._workspace("spmm", d).data_ptr())
        rc = self.lib.idg_spmm_epi_f32(graph._h, X.data_ptr(), d, d, self.C.byref(e), None if out_rows is None else out_rows.data_ptr(),
                                       None if x_rows is None else x_rows.data_ptr(), ws[1], self.ops._stream())
        if rc:
            self.check(rc, "idg_spmm_epi_f32")

    # ---- 24-bit panels (Packed24Comm): values in, 3/4 as many 32-bit words out (buffers are fp32-typed: what the comms move)
    def pack24(self, src, dst, n):
        rc = self.lib.idg_pack24_f32(src.data_ptr(), dst.data_ptr(), n, self.ops._stream())
        if rc:
            self.check(rc, "idg_pack24_f32")

    def unpack24(self, src, dst, n):
        rc = self.lib.idg_unpack24_f32(src.data_ptr(), dst.data_ptr(), n, self.ops._stream())
        if rc:
            self.check(rc, "idg_unpack24_f32")

    def reduce24(self, blocks, n_blocks, n, out_packed=None, out_f32=None):
        rc = self.lib.idg_reduce24_f32(blocks.data_ptr(), n_blocks, n, None if out_packed is None else out_packed.data_ptr(),
                                       None if out_f32 is None else out_f32.data_ptr(), self.ops._stream())
        if rc:
            self.check(rc, "idg_reduce24_f32")

    def reduce_blocks(self, blocks, n_blocks, n, out):
        rc = self.lib.idg_reduce_blocks_f32(blocks.data_ptr(), n_blocks, n, out.data_ptr(), self.ops._stream())
        if rc:
            self.check(rc, "idg_reduce_blocks_f32")

    def exchange_stream(self):
        """Context manager: what is launched (and what collective is issued) inside goes to the exchange's own stream —
        NOT ordered behind the step's stream: the caller orders it by waiting for the collectives it consumes."""
        if getattr(self, "_xchg", None) is None:
            self._xchg = self.torch.cuda.Stream()
        return self.torch.cuda.stream(self._xchg)

    def record_event(self):
        """An event on the current stream (inside exchange_stream(): the exchange's), for wait_event()."""
        ev = self.torch.cuda.Event()
        ev.record()
        return ev

    def wait_event(self, ev):
        if ev is not None:
            self.torch.cuda.current_stream().wait_event(ev)

    def bits_from(self, bits, row0):
        """The bitmap of rows row0, row0 + 1, ... (row0 a multiple of 32)."""
        if row0 == 0:
            return bits
        key = (bits.data_ptr(), row0)
        v = self._bits.get(key)
        if v is None:
            v = self._bits[key] = (bits, bits[row0 // 32:])  # (holds the base: the key's address stays its)
        return v[1]

    def ones_bits(self, n_bits):
        return self.torch.full(((n_bits + 31) // 32 + 1,), -1, dtype=self.torch.int32, device=self.device)

    def bpr(self, fin, ego, n_users, users, pos, neg, reg_lambda, g_final, g_ego, loss, prep=None):
        if prep is not None:  # the sorted (row, slot) plan is in the prepared workspace; reached rows are STORED
            prep.done.wait(self.ops._stream())
            self.ops.bpr_fused_raw(fin, ego, users, pos, neg, n_users, reg_lambda, g_final, g_ego, loss=loss, deterministic=2,
                                   touched=prep.bpr_bits, ws=prep.ws)
        else:
            self.ops.bpr_fused_raw(fin, ego, users, pos, neg, n_users, reg_lambda, g_final, g_ego, loss=loss, deterministic=1)

    def to_device(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def gather_rows(self, dst, src, idx):
        rc = self.lib.idg_rows_gather_f32(dst.data_ptr(), src.data_ptr(), idx.data_ptr(), idx.shape[0], dst.shape[1],
                                          self.ops._stream())
        if rc:
            self.check(rc, "idg_rows_gather_f32")

    def gather_rows2(self, dst0, src0, dst1, src1, idx):
        rc = self.lib.idg_rows_gather2_f32(dst0.data_ptr(), src0.data_ptr(), dst1.data_ptr(), src1.data_ptr(), idx.data_ptr(),
                                           idx.shape[0], dst0.shape[1], self.ops._stream())
        if rc:
            self.check(rc, "idg_rows_gather2_f32")

    def scatter_rows(self, dst, idx, src):
        """dst[idx[j]] = src[j] (idx distinct)."""
        self.ops.rows_scatter_raw(dst, idx, src)

    def chain_rows2(self, dst0, src0, dst1, src1, idx, nxt, store):
        if store:
            rc = self.lib.idg_rows_chain_store2_f32(dst0.data_ptr(), src0.data_ptr(), dst1.data_ptr(), src1.data_ptr(),
                                                    idx.data_ptr(), nxt.data_ptr(), idx.shape[0], dst0.shape[1],
                                                    self.ops._stream())
            if rc:
                self.check(rc, "idg_rows_chain_store2_f32")
        else:
            self.ops.rows_chain_add_raw(dst0, src0, idx, nxt)
            self.ops.rows_chain_add_raw(dst1, src1, idx, nxt)

    def layer_mean(self, out, ids, terms, last, div):
        self.ops.rows_layer_mean_raw(out, ids, terms, last, div)

    def item_tail(self, t, g, G, live_bits, row0, c0, cnt, store_grad, p, m, v, lr, step):
        rc = self.lib.idg_grad_tail_adam_f32(t.data_ptr(), g.data_ptr(), G.data_ptr(), live_bits.data_ptr(), row0, t.shape[0],
                                             t.shape[1], c0, cnt, 1 if store_grad else 0, p.data_ptr(), m.data_ptr(),
                                             v.data_ptr(), lr, 0.9, 0.999, 1e-8, step, self.ops._stream())
        if rc:
            self.check(rc, "idg_grad_tail_adam_f32")

    def adam(self, p, g, m, v, lr, step):
        self.ops.adam_step_raw(p, g, m, v, lr, step)

    # ---- the touched items (ShardedEngine._agree_touched_items) and the users near the batch's items
    def touched_local(self, eng, prep, gb):
        """One rank: the bitmap of the touched items from this rank's rows alone, and the near users."""
        # (a torch-side write of a bitmap: allowed here because nothing is ever registered for touched_buf at world size 1 —
        #  its unit lists are built by touched_from_ids, which only runs on several ranks — and mark_cols below is a library
        #  write of the same bitmap, which drops whatever was)
        prep.touched_buf.copy_(prep.items)
        eng.G_ui.mark_cols(prep.own_users, prep.touched_buf)
        prep.touched = prep.touched_buf
        self._near_users(eng, prep, gb)

    def flag_touched_items(self, eng, prep, gb, flags):
        """flags[i] = 1 for the items the batch's OWNED users interacted with, and for the batch's own items."""
        flags.zero_()
        eng.G_ui.flag_cols(prep.own_users, flags)
        flags.index_fill_(0, gb.items, 1.0)

    def nonzero_ids(self, flags):
        """Ascending ids of the non-zero flags and their number (a host synchronisation: the caller sizes a collective)."""
        ids = self.torch.nonzero(flags).reshape(-1)
        return ids, int(ids.numel())

    def compact_ids(self, flags, n):
        """Ascending ids of the non-zero flags in a list of n slots (the tail repeats the last id): built on the device,
        nothing read back (idg_flags_compact_f32)."""
        key = ("compact", flags.data_ptr())
        buf = self._ws.get(key)
        if buf is None or buf[0].shape[0] < n:
            ids, ws = self.ops.flags_compact_raw(flags, n)
            self._ws[key] = (ids, ws, flags)
            return ids
        ids = buf[0][:n]
        self.ops.flags_compact_raw(flags, n, ids=ids, ws=buf[1])
        return ids

    def touched_from_ids(self, eng, prep, ids, n):
        ids = ids[:n]
        self.ops.bpr_touch_rows_raw(ids, ids, ids, 0, prep.touched_buf, clear_bits=eng.Ip)
        prep.touched = prep.touched_buf
        # n is known here (and bounded by the compact buffer): the products restricted to the touched items — layer K - 1's
        # item side, the first backward product — run one wave per live work unit instead of visiting every tile
        st = self.ops._stream()
        for j, (g, r0, r1, r1p) in enumerate(eng.slices):
            ws = self._units(prep, ("t", j), g, eng.CS.shape[0])
            self.check(self.lib.idg_graph_live_units(g._h, self.bits_from(prep.touched_buf, r0).data_ptr(), ws.data_ptr(),
                                                     eng.CS.shape[0], st), "idg_graph_live_units")
        self._near_users(eng, prep, None)

    def _near_users(self, eng, prep, gb):
        """prep.near = the owned users that interacted with one of the batch's items, plus the owned batch users: where
        layer K - 1's user rows are read (by the last item-side product, restricted to the batch's items, and by FIN at
        the batch's users) and where the first backward product's user-side output lives."""
        prep.near_buf.copy_(prep.own_users)
        for g, r0, r1, r1p in eng.slices:
            g.mark_cols(self.bits_from(prep.items, r0), prep.near_buf)
        prep.near = prep.near_buf

    def _units(self, prep, key, graph, max_rows):
        ws = prep.units.get(key)
        if ws is None:
            nbytes = int(self.lib.idg_graph_live_units_bytes(graph._h, int(max_rows)))
            ws = prep.units[key] = self.torch.empty(nbytes // 4, dtype=self.torch.int32, device=self.device)
        return ws

    def topk(self, user_panel, item_panel, users, k, excl_indptr, excl_items):
        """Top-k item ids [len(users), k] (numpy) for local user ids `users`, train items excluded."""
        torch = self.torch
        idx = self.ops.score_topk(user_panel, item_panel, self.to_device(np.asarray(users, dtype=np.int64)), int(k),
                                  self.to_device(np.asarray(excl_indptr, dtype=np.int64)),
                                  self.to_device(np.asarray(excl_items, dtype=np.int32)), apply_sigmoid=True)
        torch.cuda.synchronize()
        return idx.cpu().numpy()

    class _Prepared:
        __slots__ = ("own_users", "items", "touched_buf", "near_buf", "touched", "near", "bpr_bits", "ws", "rows_done", "done",
                     "B", "busy", "units", "graphs", "args", "tables", "owner")

    def prepare(self, eng, gb):
        """Index-only work of a global batch on a side stream: the bitmap of the LOCAL user rows this rank owns in it,
        the bitmap of the batch's item rows (ALL triples' positives and negatives: every rank evaluates the whole batch),
        their lists of live work units (the last forward layer runs one wave per unit: idg_graph_live_units), a cleared
        bitmap for the gradient scatter to flag its stored rows in, and the sorted scatter plan of the whole batch over
        the guest rows.  Host cost matters here: raw stream handles and events allocated once."""
        torch, ops, lib = self.torch, self.ops, self.lib
        cap, n_users, n, d = eng.B, eng.Ug + eng.B, eng.Ug + eng.B + eng.Ip, eng.d
        # (pooled per ENGINE: the cached arguments hold that engine's graph handles, slice tables and bitmap sizes — ADVICE r03)
        prep = next((p for p in self._pool if p.owner is eng and p.B == cap and not p.busy), None)
        if prep is None:
            prep = self._Prepared()
            prep.owner = eng
            words = lambda bits: torch.zeros((bits + 31) // 32 + 1, dtype=torch.int32, device=self.device)  # noqa: E731
            prep.own_users, prep.near_buf = words(eng.Ug), words(eng.Ug)
            prep.items, prep.touched_buf = words(eng.Ip), words(eng.Ip)
            prep.bpr_bits = words(n)
            prep.ws, prep.B = ops.bpr_workspace(cap, d, self.device), cap
            prep.rows_done, prep.done = ops.LocalEvent(), ops.LocalEvent()  # device-local events
            prep.units = {}
            prep.graphs = [eng.G_ui] + [sl[0] for sl in eng.slices]  # (their unit lists name this object's bitmaps)
            C, S = self.C, len(eng.slices)
            a = prep.args = self.ShardPrep()
            a.guest_ids, a.B_cap = eng.guest_ids.data_ptr(), cap
            a.users_bits, a.n_local_users = prep.own_users.data_ptr(), eng.Ug
            a.items_bits, a.n_items_padded = prep.items.data_ptr(), eng.Ip
            a.scatter_bits, a.n_panel_rows = prep.bpr_bits.data_ptr(), n
            a.user_graph, a.user_units = eng.G_ui._h, self._units(prep, "u", eng.G_ui, cap).data_ptr()
            a.n_slices = S
            prep.tables = ((C.c_void_p * S)(*[sl[0]._h.value for sl in eng.slices]), (C.c_int64 * S)(*[sl[1] for sl in eng.slices]),
                           (C.c_void_p * S)(*[self._units(prep, ("i", j), sl[0], 2 * cap).data_ptr() for j, sl in enumerate(eng.slices)]))
            a.slice_graphs, a.slice_row0, a.slice_units = prep.tables
            a.plan_ws = prep.ws.data_ptr()
            a.side_stream = self._side_raw
            a.ev_fork, a.ev_rows, a.ev_plan = self._fork._h, prep.rows_done._h, prep.done._h
            self._pool.append(prep)
        prep.busy = True
        prep.touched = prep.near = None
        # one library call for the whole preparation (idg_shard_prepare); only the batch's own arrays change per call
        a = prep.args
        a.own_users, a.n_own = (gb.own_users.data_ptr() if gb.n_owned > 0 else None), gb.n_owned
        a.pos, a.neg, a.B = gb.pos.data_ptr(), gb.neg.data_ptr(), gb.B
        a.main_stream = ops._stream()
        rc = lib.idg_shard_prepare(self.C.byref(a))
        if rc:
            self.check(rc, "idg_shard_prepare")
        return prep

    def wait_rows(self, prep):
        """The bitmaps are first read by a product on the main stream."""
        prep.rows_done.wait(self.ops._stream())

    def release(self, prep):
        prep.busy = False  # its buffers go back to the pool; reuse is ordered by the fork event of the next prepare()

    def close(self):
        """The pooled bitmaps and unit lists die with this object: nothing may stay registered under their addresses.
        Called by whoever owns the engine when it is done (the bench does); __del__ is only the safety net."""
        for prep in self._pool:
            for ws in prep.units.values():
                self.lib.idg_graph_forget_units_ws(ws.data_ptr())
            for g in prep.graphs:
                g.forget_live_units()
        self._pool = []

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
