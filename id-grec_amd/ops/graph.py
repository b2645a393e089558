"""csrc/idg_graph.hip — Graph, the products with their epilogues, the row movers, the noise streams, the propagation operators —
and, each under its section header, the families every encoder builds on: InfoNCE (idg_ssl), row normalisation, BPR, the
thin dense layer and NGCF, LR-GCCF, GCMC, IMP-GCN's groups, BIGCF's intent layer, HCCF's hypergraph layer."""
import ctypes as C
import os
import weakref

import numpy as np
import torch

from .. import native
from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ld, _ptr, _require_device, _require_ids, _row_base, _stream


def _forget_units_ws(ws_ptr):
    """Finalizer of a list buffer: whatever is registered IN that buffer goes (a newer list of the same bitmap, built into
    another buffer, stays: ADVICE r03)."""
    if lib is not None:
        lib.idg_graph_forget_units_ws(ws_ptr)


def _forget_units_of(graph_ref, bitmap_ptr):
    g = graph_ref()
    if g is not None and getattr(g, "_h", None) and lib is not None:
        lib.idg_graph_forget_live_units(g._h, bitmap_ptr)


class Graph:
    """Device-resident CSR adjacency + its row-block tile schedule (idg_graph).

    Built from HOST CSR arrays (numpy / scipy).  `symmetric=True` declares A == A^T so the
    backward pass reuses the same handle (true for the normalised bipartite adjacency,
    SURVEY §0.6); otherwise the transposed CSR is built once on the host.
    """

    def __init__(self, indptr, indices, values, n_rows, n_cols, device=None, symmetric=True, exact_order=False,
                 split_threshold=0, build_transpose=True, _transpose_of=None, balanced_tiles=True):
        if not torch.cuda.is_available():
            raise RuntimeError("idgrec_amd.Graph needs a HIP device (torch.cuda.is_available() is False); "
                               "this library has no CPU path.")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("idgrec_amd.Graph: device must be a cuda(HIP) device, got %s" % dev)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.float32)
        self.nnz = int(indices.shape[0])
        self.symmetric = bool(symmetric)
        flags = (native.IDG_GRAPH_SYMMETRIC if symmetric else 0) | (native.IDG_GRAPH_EXACT_ORDER if exact_order else 0) \
            | (0 if balanced_tiles else native.IDG_GRAPH_NO_BALANCED)
        h = C.c_void_p()
        check(lib.idg_graph_create(self.device.index, self.n_rows, self.n_cols, self.nnz,
                                   native.np_ptr(indptr, C.c_int64), native.np_ptr(indices, C.c_int32),
                                   native.np_ptr(values, C.c_float), flags, int(split_threshold), C.byref(h)),
              "idg_graph_create")
        self._h = h
        self._ws = {}
        self._T = _transpose_of
        if not symmetric and build_transpose and _transpose_of is None:
            import scipy.sparse as sp

            At = sp.csr_matrix((values, indices, indptr), shape=(self.n_rows, self.n_cols)).T.tocsr()
            At.sort_indices()
            self._T = Graph(At.indptr, At.indices, At.data, self.n_cols, self.n_rows, device=self.device,
                            symmetric=False, exact_order=exact_order, split_threshold=split_threshold,
                            _transpose_of=self, balanced_tiles=balanced_tiles)

    @classmethod
    def from_torch_sparse(cls, t, symmetric=True, exact_order=False, split_threshold=0, balanced_tiles=True):
        """From the reference's own operand: a coalesced sparse COO (or CSR) fp32 tensor that lives on the device
        (models/LightGCN.py:31-32: convert_sp_mat_to_sp_tensor(...).coalesce().to(device)) — idg_graph_create_from_device.
        Non-symmetric graphs get no transposed handle here (build it from t.t().coalesce())."""
        if not t.is_cuda:
            raise RuntimeError("Graph.from_torch_sparse needs a device tensor; idgrec_amd has no CPU path")
        csr = t if t.layout == torch.sparse_csr else t.coalesce().to_sparse_csr()
        crow = csr.crow_indices().to(torch.int64).contiguous()
        col = csr.col_indices().to(torch.int32).contiguous()
        val = csr.values().to(torch.float32).contiguous()
        g = cls.__new__(cls)
        g.device, (g.n_rows, g.n_cols), g.nnz = t.device, (int(t.shape[0]), int(t.shape[1])), int(col.shape[0])
        g.symmetric, g._ws, g._T = bool(symmetric), {}, None
        flags = (native.IDG_GRAPH_SYMMETRIC if symmetric else 0) | (native.IDG_GRAPH_EXACT_ORDER if exact_order else 0) \
            | (0 if balanced_tiles else native.IDG_GRAPH_NO_BALANCED)
        h = C.c_void_p()
        with torch.cuda.device(t.device):
            check(lib.idg_graph_create_from_device(t.device.index, g.n_rows, g.n_cols, g.nnz, _ptr(crow), _ptr(col), _ptr(val),
                                                   flags, int(split_threshold), _stream(), C.byref(h)),
                  "idg_graph_create_from_device")
        g._h = h
        return g

    @classmethod
    def from_scipy(cls, mat, **kw):
        m = mat.tocsr()
        m.sort_indices()
        return cls(m.indptr, m.indices, m.data, m.shape[0], m.shape[1], **kw)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # module globals are already gone at interpreter shutdown
            lib.idg_graph_destroy(h)

    @property
    def T(self):
        return self if self.symmetric else self._T

    # ---- live work units of a row bitmap (idg_graph_live_units): restricted launches naming the bitmap then run one
    #      wave per unit instead of visiting every tile
    def live_units(self, bitmap, max_rows, ws=None, stream=None):
        """Build (on `stream`, default: current) and register the unit list of `bitmap` (int32 tensor); returns the
        list's buffer, which the caller keeps alive while the bitmap is in use — and re-builds whenever the bitmap's
        contents change."""
        _require_device(bitmap, ws)
        if ws is None:
            ws = torch.empty(int(lib.idg_graph_live_units_bytes(self._h, int(max_rows))) // 4, dtype=torch.int32,
                             device=self.device)
        check(lib.idg_graph_live_units(self._h, _ptr(bitmap), _ptr(ws), int(max_rows), _stream() if stream is None else stream),
              "idg_graph_live_units")
        # the registration names two caller-owned buffers: it must not outlive either (the allocator may hand the same
        # address to something else).  One finalizer per tensor object, however often the list is rebuilt.
        # (the bitmap's finalizer forgets by bitmap, the list buffer's by buffer: a dying OLD buffer must not take a NEW
        #  registration of the same bitmap with it)
        if not getattr(bitmap, "_idg_units_finalizer", False):
            weakref.finalize(bitmap, _forget_units_of, weakref.ref(self), bitmap.data_ptr())
            bitmap._idg_units_finalizer = True
        if not getattr(ws, "_idg_units_finalizer", False):
            weakref.finalize(ws, _forget_units_ws, ws.data_ptr())
            ws._idg_units_finalizer = True
        return ws

    @staticmethod
    def live_units_check(ws, stream=None):
        """Raises if the list in `ws` could not hold every row of its bitmap (idg_graph_live_units_check; synchronises)."""
        check(lib.idg_graph_live_units_check(_ptr(ws), _stream() if stream is None else stream), "idg_graph_live_units_check")

    def compact_inputs(self, bitmap, ws=None, stream=None):
        """idg_graph_compact_inputs: the tiles' entry lists compacted to the live INPUT rows of `bitmap`, built on `stream`
        and registered for it; a product naming the bitmap as x_rows / gout mask then walks them.  Returns the buffer
        (keep it alive while the bitmap is in use; pass it back to rebuild in place)."""
        _require_device(bitmap, ws)
        if ws is None:
            ws = torch.empty(int(lib.idg_graph_compact_inputs_bytes(self._h)), dtype=torch.uint8, device=self.device)
        check(lib.idg_graph_compact_inputs(self._h, _ptr(bitmap), _ptr(ws), _stream() if stream is None else stream),
              "idg_graph_compact_inputs")
        # (the bitmap's finalizer forgets by bitmap, the list buffer's by buffer: a dying OLD buffer must not take a NEW
        #  registration of the same bitmap with it)
        if not getattr(bitmap, "_idg_units_finalizer", False):
            weakref.finalize(bitmap, _forget_units_of, weakref.ref(self), bitmap.data_ptr())
            bitmap._idg_units_finalizer = True
        if not getattr(ws, "_idg_units_finalizer", False):
            weakref.finalize(ws, _forget_units_ws, ws.data_ptr())
            ws._idg_units_finalizer = True
        return ws

    def bind_live_units(self, bitmap, ws, max_rows):
        """Register an existing list (built on a handle with the same schedule: the base of a masked / revalued copy)."""
        check(lib.idg_graph_bind_live_units(self._h, _ptr(bitmap), _ptr(ws), int(max_rows)), "idg_graph_bind_live_units")

    def forget_live_units(self, bitmap=None):
        if getattr(self, "_h", None):
            lib.idg_graph_forget_live_units(self._h, _ptr(bitmap))

    def revalued_copy(self, d_indptr, d_indices, d_values):
        """A Graph on this handle's structure and tile schedule with the values of the DEVICE CSR (d_indptr int64,
        d_indices int32, d_values fp32) — idg_graph_revalued_copy.  No host work: SGL's per-epoch edge-dropped views."""
        _require_device(d_indptr, d_indices, d_values)
        if d_indptr.dtype != torch.int64 or d_indices.dtype != torch.int32 or d_values.dtype != torch.float32:
            raise TypeError("revalued_copy: indptr int64, indices int32, values float32")
        g = Graph.__new__(Graph)
        g.device, g.n_rows, g.n_cols, g.nnz, g.symmetric = self.device, self.n_rows, self.n_cols, self.nnz, self.symmetric
        g._ws, g._base, g._T = self._ws, self, None
        h = C.c_void_p()
        check(lib.idg_graph_revalued_copy(self._h, _ptr(d_indptr), _ptr(d_indices), _ptr(d_values), _stream(), C.byref(h)),
              "idg_graph_revalued_copy")
        g._h = h
        return g

    def dropout_copy(self, keep_prob, stream=None, reuse=None):
        """NGCF.node_dropout (models/NGCF.py:56-65) of a SYMMETRIC graph as a new Graph on the same tile schedule:
        every stored entry is kept where int(u + (1 - keep_prob)) != 0, u ~ U[0, 1) — i.e. with probability
        1 - keep_prob, the reference's own (inverted-looking) rule — and divided by (1 - keep_prob); its `.T` (used by
        the backward of spmm) carries the transposed mask.  stream: (seed, stream id) of the draw; default: the next
        one of the device seed's sequence.  reuse: a Graph an earlier call on this handle returned — its two entry
        lists are redrawn in place (no allocation, nothing synchronous: the per-forward form)."""
        if not self.symmetric:
            raise ValueError("dropout_copy needs a symmetric graph (the transposed mask is read off the same structure)")
        seed, sid = _next_noise_stream() if stream is None else stream
        add = 1.0 - float(keep_prob)
        if reuse is not None and getattr(reuse, "_base", None) is self and reuse._T is not None:
            for g, transpose in ((reuse, 0), (reuse._T, 1)):
                check(lib.idg_graph_remask(self._h, g._h, add, add, C.c_uint64(seed), C.c_uint64(sid), transpose, _stream()),
                      "idg_graph_remask")
            return reuse
        out = []
        for transpose in (0, 1):
            g = Graph.__new__(Graph)
            g.device, g.n_rows, g.n_cols, g.nnz, g.symmetric = self.device, self.n_rows, self.n_cols, self.nnz, False
            g._ws, g._base = self._ws, self  # same workspaces (same schedule); keeps the base handle alive
            h = C.c_void_p()
            check(lib.idg_graph_masked_copy(self._h, add, add, C.c_uint64(seed), C.c_uint64(sid), transpose, _stream(),
                                            C.byref(h)), "idg_graph_masked_copy")
            g._h = h
            out.append(g)
        out[0]._T, out[1]._T = out[1], out[0]
        return out[0]

    def info(self):
        a = (C.c_int64 * 8)()
        check(lib.idg_graph_info(self._h, a), "idg_graph_info")
        keys = ("n_rows", "n_cols", "nnz", "n_tiles", "n_long_rows", "n_segments", "split_threshold", "flags")
        return dict(zip(keys, [int(x) for x in a]))

    def schedule_info(self):
        """idg_graph_schedule_info: {"base": {...}, "balanced": {...}} with tiles, rounds, slots (16 x makespan summed over
        the tiles), bytes and utilisation = rounds / slots of the handle's two tile schedules (balanced: zeros when the
        handle carries none).  Reads the schedule back from the device."""
        a = (C.c_int64 * 8)()
        check(lib.idg_graph_schedule_info(self._h, a), "idg_graph_schedule_info")
        out = {}
        for name, o in (("base", 0), ("balanced", 4)):
            tiles, rounds, slots, nbytes = (int(a[o + k]) for k in range(4))
            out[name] = {"tiles": tiles, "rounds": rounds, "slots": slots, "bytes": nbytes,
                         "utilisation": rounds / slots if slots else 0.0}
        return out

    def long_rows(self):
        n = self.info()["n_long_rows"]
        rows = np.empty(n, dtype=np.int64)
        seg = np.empty(n, dtype=np.int64)
        chunk = np.empty(n, dtype=np.int64)
        check(lib.idg_graph_long_rows(self._h, native.np_ptr(rows, C.c_int64), native.np_ptr(seg, C.c_int64),
                                      native.np_ptr(chunk, C.c_int64)), "idg_graph_long_rows")
        return rows, seg, chunk

    def _workspace(self, kind, d):
        fn = lib.idg_spmm_workspace_bytes if kind == "spmm" else lib.idg_propagate_workspace_bytes
        return _cached_ws(self._ws, (kind, int(d)), lambda: max(int(fn(self._h, int(d))), 16), self.device)

    # ---- raw (non-autograd) calls
    def spmm_raw(self, X, addend=None, out=None):
        _require_device(X, addend, out)
        # a column slice of a wider contiguous panel (row stride ldx, unit column stride) is read where it lies:
        # idg_spmm_f32 takes the leading dimension (LR-GCCF's layers live only in their slots of the final panel)
        in_place = X.dim() == 2 and X.dtype == torch.float32 and not X.is_contiguous() and X.stride(1) == 1 \
            and X.stride(0) >= X.shape[1]
        if not in_place:
            X = _f32c(X, "X")
        if X.dim() != 2 or X.shape[0] != self.n_cols:
            raise ValueError("X must be [%d, d], got %s" % (self.n_cols, tuple(X.shape)))
        d = X.shape[1]
        ldx = X.stride(0) if in_place else d
        Y = torch.empty((self.n_rows, d), dtype=torch.float32, device=X.device) if out is None else out
        if addend is not None:
            addend = _f32c(addend, "addend")
            if addend.shape != Y.shape:
                raise ValueError("addend shape %s != output shape %s" % (tuple(addend.shape), tuple(Y.shape)))
        ws = self._workspace("spmm", d)
        check(lib.idg_spmm_f32(self._h, _ptr(X), ldx, _ptr(Y), d, _ptr(addend), d, _ptr(ws), _stream()), "idg_spmm_f32")
        return Y

    def propagate_mean_raw(self, E0, K, include_layer0=True, out=None, out_rows=None):
        """out_rows: int32 bitmap tensor of the rows of the result that will be read (others are left
        untouched), or None for the whole panel."""
        _require_device(E0, out, out_rows)
        E0 = _f32c(E0, "E0")
        if E0.shape[0] != self.n_rows:
            raise ValueError("E0 must have %d rows, got %d" % (self.n_rows, E0.shape[0]))
        d = E0.shape[1]
        out = torch.empty_like(E0) if out is None else out
        ws = self._workspace("prop", d)
        check(lib.idg_propagate_mean_f32(self._h, _ptr(E0), _ptr(out), _ptr(out_rows), int(K), int(bool(include_layer0)),
                                         d, _ptr(ws), _stream()), "idg_propagate_mean_f32")
        return out

    def propagate_mean_noise_raw(self, E0, K, include_layer0, eps, seed, stream_id, out=None, out_rows=None):
        """idg_propagate_mean_noise_f32 (SimGCL's perturbed encoder pass); out_rows as in propagate_mean_raw."""
        _require_device(E0, out, out_rows)
        E0 = _f32c(E0, "E0")
        d = E0.shape[1]
        out = torch.empty_like(E0) if out is None else out
        ws = self._workspace("prop", d)
        check(lib.idg_propagate_mean_noise_f32(self._h, _ptr(E0), _ptr(out), _ptr(out_rows), int(K), int(bool(include_layer0)),
                                               d, float(eps), C.c_uint64(seed), C.c_uint64(stream_id), _ptr(ws), _stream()),
              "idg_propagate_mean_noise_f32")
        return out

    def propagate_mean_bwd_raw(self, gout, K, include_layer0=True, out=None, accumulate=False, mask=None):
        """mask: int32/uint32 bitmap tensor of gout's live rows (see idg_propagate_mean_bwd_f32), or None."""
        _require_device(gout, out, mask)
        gout = _f32c(gout, "gout")
        d = gout.shape[1]
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs an existing `out`")
            out = torch.empty_like(gout)
        ws = self._workspace("prop", d)
        check(lib.idg_propagate_mean_bwd_f32(self._h, _ptr(gout), _ptr(mask), _ptr(out), int(K), int(bool(include_layer0)), d,
                                             int(bool(accumulate)), _ptr(ws), _stream()),
              "idg_propagate_mean_bwd_f32")
        return out

    # ---- the batch's receptive field (idg_graph_expand_rows, idg_propagate_mean*_fields_f32)
    def expand_rows(self, in_rows, out_rows, stream=None):
        """out_rows = in_rows | neighbours of the rows flagged in in_rows (int32 bitmap tensors of n_rows bits)."""
        _require_device(in_rows, out_rows)
        check(lib.idg_graph_expand_rows(self._h, _ptr(in_rows), _ptr(out_rows), _stream() if stream is None else stream),
              "idg_graph_expand_rows")

    def flag_cols(self, in_rows, col_flags, stream=None):
        """col_flags[c] = 1.0 for the columns of the stored entries of the rows flagged in in_rows (float32 [n_cols],
        zeroed by the caller): idg_graph_flag_cols."""
        _require_device(in_rows, col_flags)
        check(lib.idg_graph_flag_cols(self._h, _ptr(in_rows), _ptr(col_flags), _stream() if stream is None else stream),
              "idg_graph_flag_cols")

    def mark_cols(self, in_rows, col_bits, stream=None):
        """col_bits |= the columns of the stored entries of the rows flagged in in_rows (int32 bitmap of n_cols bits, not
        cleared here): idg_graph_mark_cols."""
        _require_device(in_rows, col_bits)
        check(lib.idg_graph_mark_cols(self._h, _ptr(in_rows), _ptr(col_bits), _stream() if stream is None else stream),
              "idg_graph_mark_cols")

    @staticmethod
    def _bitmap_array(bitmaps):
        arr = (C.c_void_p * len(bitmaps))(*[None if b is None else b.data_ptr() for b in bitmaps])
        return arr

    def propagate_mean_fields_raw(self, E0, K, include_layer0, out, layer_rows):
        """idg_propagate_mean_fields_f32: layer k produces the rows of layer_rows[k-1] only (K bitmaps, the last = the
        batch's rows)."""
        _require_device(E0, out, *layer_rows)
        E0 = _f32c(E0, "E0")
        d = E0.shape[1]
        if len(layer_rows) != K:
            raise ValueError("layer_rows needs K bitmaps")
        ws = self._workspace("prop", d)
        check(lib.idg_propagate_mean_fields_f32(self._h, _ptr(E0), _ptr(out), self._bitmap_array(layer_rows), int(K),
                                                int(bool(include_layer0)), d, _ptr(ws), _stream()),
              "idg_propagate_mean_fields_f32")
        return out

    def propagate_mean_bwd_adam_fields_raw(self, gout, K, include_layer0, out, accumulate, step_rows, param, exp_avg,
                                           exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, discard_grad=False):
        """idg_propagate_mean_bwd_adam_fields_f32: step k's input is zero outside step_rows[k-1] (None = dense)."""
        _require_device(gout, out, param, exp_avg, exp_avg_sq, *[b for b in step_rows if b is not None])
        gout = _f32c(gout, "gout")
        d = gout.shape[1]
        if len(step_rows) != K or step_rows[0] is None:
            raise ValueError("step_rows needs K entries, the first a bitmap")
        ws = self._workspace("prop", d)
        check(lib.idg_propagate_mean_bwd_adam_fields_f32(self._h, _ptr(gout), self._bitmap_array(step_rows), _ptr(out), int(K),
                                                         int(bool(include_layer0)), d, int(bool(accumulate)) | (native.IDG_ADAM_DISCARD_GRAD if discard_grad else 0), _ptr(param),
                                                         _ptr(exp_avg), _ptr(exp_avg_sq), float(lr), float(beta1),
                                                         float(beta2), float(eps), int(step), _ptr(ws), _stream()),
              "idg_propagate_mean_bwd_adam_fields_f32")
        return out

    def propagate_mean_bwd_adam_raw(self, gout, K, include_layer0, out, accumulate, mask, param, exp_avg, exp_avg_sq, lr,
                                    step, beta1=0.9, beta2=0.999, eps=1e-8, discard_grad=False):
        """idg_propagate_mean_bwd_adam_f32: the backward above with the dense Adam step on `param` applied in the
        epilogue of its last product (bit-identical to propagate_mean_bwd_raw + adam_step_raw).  discard_grad: the
        finished gradient is not written back to `out` (IDG_ADAM_DISCARD_GRAD)."""
        _require_device(gout, out, mask, param, exp_avg, exp_avg_sq)
        gout = _f32c(gout, "gout")
        d = gout.shape[1]
        for t in (out, param, exp_avg, exp_avg_sq):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != gout.shape:
                raise TypeError("propagate_mean_bwd_adam_raw needs contiguous float32 panels shaped like gout")
        ws = self._workspace("prop", d)
        check(lib.idg_propagate_mean_bwd_adam_f32(self._h, _ptr(gout), _ptr(mask), _ptr(out), int(K), int(bool(include_layer0)),
                                                  d, int(bool(accumulate)) | (native.IDG_ADAM_DISCARD_GRAD if discard_grad else 0),
                                                  _ptr(param), _ptr(exp_avg), _ptr(exp_avg_sq),
                                                  float(lr), float(beta1), float(beta2), float(eps), int(step), _ptr(ws),
                                                  _stream()), "idg_propagate_mean_bwd_adam_f32")
        return out


def spmm_ex_raw(graph, X, Y=None, addend=None, sum_in=None, sum_out=None, div=1.0, accumulate=False, out_rows=None,
                x_rows=None):
    """idg_spmm_ex_f32: t = A.X (+ addend); Y = t; sum_out (+)= (sum_in + t) / div.  All [*, d] contiguous.
    out_rows / x_rows: optional int32 bitmaps of the output rows wanted / of the non-zero rows of X."""
    _require_device(X, Y, addend, sum_in, sum_out, out_rows, x_rows)
    d = X.shape[1]
    for t in (X, Y, addend, sum_in, sum_out):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape[1] != d):
            raise TypeError("spmm_ex_raw needs contiguous float32 [*, %d] panels" % d)
    ws = graph._workspace("spmm", d)
    check(lib.idg_spmm_ex_f32(graph._h, _ptr(X), d, _ptr(Y), _ptr(addend), _ptr(sum_in), _ptr(sum_out), d, float(div),
                              int(bool(accumulate)), _ptr(out_rows), _ptr(x_rows), d, _ptr(ws), _stream()), "idg_spmm_ex_f32")


def spmm_epi_raw(graph, X, Y=None, addend=None, sum_in=None, sum_in2=None, sum_in3=None, sum_out=None, div=1.0,
                 accumulate=False, mask=None, adam=None, out_rows=None, x_rows=None, adam_discard_grad=False, act=0,
                 act_src=None, act_rows=0):
    """idg_spmm_epi_f32: the product with every epilogue option (include/idgrec.h, idg_epilogue).  mask: bitmap of the
    live rows of addend / sum_in* / the accumulate target; adam = (param, exp_avg, exp_avg_sq, lr, step[, beta1, beta2,
    eps]): the Adam update of the rows of `param` with gradient sum_out in the same launch (adam_discard_grad: without
    writing that gradient).  out_rows and x_rows may be combined.  act: native.ACT_TANH (t = tanh(t)) or
    native.ACT_TANH_BWD (t *= 1 - act_src^2) applied to the rows below act_rows (0: all) before anything is stored."""
    _require_device(X, Y, addend, sum_in, sum_in2, sum_in3, sum_out, mask, out_rows, x_rows, act_src)
    d = X.shape[1]
    for t in (X, Y, addend, sum_in, sum_in2, sum_in3, sum_out):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape[1] != d):
            raise TypeError("spmm_epi_raw needs contiguous float32 [*, %d] panels" % d)
    e = native.Epilogue(_ptr(Y), _ptr(addend), _ptr(sum_in), _ptr(sum_in2), _ptr(sum_in3), _ptr(sum_out), d, float(div),
                        int(bool(accumulate)), _ptr(mask))
    if adam is not None:
        p, m, v, lr, step = adam[:5]
        b1, b2, eps = (tuple(adam[5:8]) + (0.9, 0.999, 1e-8)[len(adam) - 5:])[:3] if len(adam) > 5 else (0.9, 0.999, 1e-8)
        _require_device(p, m, v)
        e.adam_param, e.adam_exp_avg, e.adam_exp_avg_sq = _ptr(p), _ptr(m), _ptr(v)
        e.adam_lr, e.adam_beta1, e.adam_beta2, e.adam_eps, e.adam_step = float(lr), float(b1), float(b2), float(eps), int(step)
        e.adam_discard_grad = int(bool(adam_discard_grad))
    if act:
        e.act, e.act_src, e.act_rows = int(act), _ptr(act_src), int(act_rows)
    ws = graph._workspace("spmm", d)
    check(lib.idg_spmm_epi_f32(graph._h, _ptr(X), d, d, C.byref(e), _ptr(out_rows), _ptr(x_rows), _ptr(ws), _stream()),
          "idg_spmm_epi_f32")


_ssl_ws = {}  # InfoNCE workspaces by (n, B, d, device): the pair and cross forms of one step share one


def rows_tanh_bwd_raw(grad, y, rows, out):
    """out[r] = grad[r] * (1 - y[r]^2) at the rows of the bitmap `rows` (None: all) — idg_rows_tanh_bwd_f32."""
    _require_device(grad, y, rows, out)
    check(lib.idg_rows_tanh_bwd_f32(_ptr(grad), _ptr(y), _ptr(rows), int(grad.shape[0]), int(grad.shape[1]), _ptr(out), _stream()),
          "idg_rows_tanh_bwd_f32")


SSL_UNIQUE, SSL_RAW, SSL_CROSS = 0, 1, 2  # idg_infonce_plan modes


def infonce_workspace(n, B, d, device):
    """A workspace of idg_infonce_*_f32 for [n, d] panels and batches of B ids (one per batch in flight)."""
    return torch.empty(int(lib.idg_infonce_workspace_bytes(int(n), int(B), int(d))), dtype=torch.uint8, device=device)


def infonce_plan_raw(users, items, num_users, n, d, mode, ws, stream=None):
    """idg_infonce_plan: the id-list stage of an InfoNCE call (index-only work) into `ws`, on `stream` (raw handle; default:
    the current stream) — then infonce_pair_raw / infonce_cross_raw(..., ws=ws, planned=True) on the stream that has
    waited for it."""
    _require_device(users, items, ws)
    _require_ids(users, items)
    check(lib.idg_infonce_plan(_ptr(users), _ptr(items), users.shape[0], int(num_users), int(n), int(d), int(mode), _ptr(ws),
                               _stream() if stream is None else stream), "idg_infonce_plan")


def infonce_cross_raw(view, users, items, num_users, temperature, g=None, loss=None, grad_scale=1.0, ws=None, planned=False):
    """get_InfoNCE_loss(view[users], view[num_users + items], t) on the raw batch rows (models/EGCF.py:103), forward and
    backward: loss [1] and the gradient rows ADDED into g (idg_infonce_cross_f32).  Returns (loss, ws)."""
    _require_device(view, users, items, g, loss, ws)
    n, d = view.shape
    B = int(users.shape[0])
    if loss is None:
        loss = torch.zeros(2, dtype=torch.float32, device=view.device)
    if ws is None:
        ws = _cached_ws(_ssl_ws, (n, B, d, view.device), lambda: lib.idg_infonce_workspace_bytes(n, B, d), view.device)
    check(lib.idg_infonce_cross_ex_f32(_ptr(view), n, d, _ptr(users), _ptr(items), B, int(num_users), float(temperature), _ptr(loss),
                                       _ptr(g), float(grad_scale), int(bool(planned)), _ptr(ws), _stream()), "idg_infonce_cross_f32")
    return loss, ws


def rows_gather2_raw(dst0, src0, dst1, src1, idx):
    """dstP[t] = srcP[idx[t]] (zeros where idx[t] < 0) for two panel pairs in one launch (idg_rows_gather2_f32)."""
    _require_device(dst0, src0, dst1, src1, idx)
    check(lib.idg_rows_gather2_f32(_ptr(dst0), _ptr(src0), _ptr(dst1), _ptr(src1), _ptr(idx), int(idx.shape[0]),
                                   int(dst0.shape[1]), _stream()), "idg_rows_gather2_f32")


def rows_scatter_raw(dst, idx, src):
    """dst[idx[j]] = src[j] (idg_rows_scatter_f32)."""
    _require_device(dst, idx, src)
    check(lib.idg_rows_scatter_f32(_ptr(dst), _ptr(idx), _ptr(src), int(src.shape[0]), int(dst.shape[1]), _stream()),
          "idg_rows_scatter_f32")


def rows_chain_store2_raw(dst0, src0, dst1, src1, idx, nxt):
    """dstP[idx[t]] = srcP[t] + srcP[nxt[t]] + ... for every head t, stored (idg_rows_chain_store2_f32)."""
    _require_device(dst0, src0, dst1, src1, idx, nxt)
    check(lib.idg_rows_chain_store2_f32(_ptr(dst0), _ptr(src0), _ptr(dst1), _ptr(src1), _ptr(idx), _ptr(nxt),
                                        int(idx.shape[0]), int(dst0.shape[1]), _stream()), "idg_rows_chain_store2_f32")


def rows_layer_mean_raw(out, ids, terms, last, div):
    """out[ids[j]] = (((a + b) + c)[ids[j]] + last[j]) / div, terms = up to three panels (idg_rows_layer_mean_f32); more
    terms (K > 3 layers), added left to right the same way: idg_rows_layer_mean_n_f32."""
    terms = [t for t in terms if t is not None]
    _require_device(out, ids, last, *terms)
    if len(terms) > 3:
        arr = (C.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
        check(lib.idg_rows_layer_mean_n_f32(_ptr(out), _ptr(ids), int(ids.shape[0]), arr, len(terms), _ptr(last), float(div),
                                            int(out.shape[1]), _stream()), "idg_rows_layer_mean_n_f32")
        return
    a, b, c = (terms + [None, None, None])[:3]
    check(lib.idg_rows_layer_mean_f32(_ptr(out), _ptr(ids), int(ids.shape[0]), _ptr(a), _ptr(b), _ptr(c), _ptr(last),
                                      float(div), int(out.shape[1]), _stream()), "idg_rows_layer_mean_f32")


def grad_tail_adam_raw(t, g, G, live_bits, row0, include_layer0, cnt, store_grad, param, exp_avg, exp_avg_sq, lr, step,
                       beta1=0.9, beta2=0.999, eps=1e-8):
    """idg_grad_tail_adam_f32 on a block of rows: every tensor is the block's [rows, d] slice of its panel."""
    _require_device(t, g, G, live_bits, param, exp_avg, exp_avg_sq)
    check(lib.idg_grad_tail_adam_f32(_ptr(t), _ptr(g), _ptr(G), _ptr(live_bits), int(row0), int(t.shape[0]), int(t.shape[1]),
                                     int(bool(include_layer0)), float(cnt), int(bool(store_grad)), _ptr(param),
                                     _ptr(exp_avg), _ptr(exp_avg_sq), float(lr), float(beta1), float(beta2), float(eps),
                                     int(step), _stream()), "idg_grad_tail_adam_f32")


def lincomb_raw(out, x, a, y=None, b=0.0):
    """out = a*x + b*y (y may be None)."""
    _require_device(out, x, y)
    check(lib.idg_lincomb_f32(_ptr(out), _ptr(x), float(a), _ptr(y), float(b), out.numel(), _stream()), "idg_lincomb_f32")


def subgraph_values_raw(row_of_entry, col_of_entry, edge_of_entry, kept_bits, dinv, out=None):
    """idg_subgraph_values_f32: the normalised values of an edge-dropped bipartite adjacency, in CSR entry order."""
    _require_device(row_of_entry, col_of_entry, edge_of_entry, kept_bits, dinv, out)
    nnz = row_of_entry.shape[0]
    out = torch.empty(nnz, dtype=torch.float32, device=dinv.device) if out is None else out
    check(lib.idg_subgraph_values_f32(nnz, _ptr(row_of_entry), _ptr(col_of_entry), _ptr(edge_of_entry), _ptr(kept_bits),
                                      _ptr(dinv), _ptr(out), _stream()), "idg_subgraph_values_f32")
    return out


def flags_compact_raw(flags, cap, ids=None, count=None, ws=None):
    """ids[0..cap) = ascending indices of the non-zero entries of the float vector `flags`, slots past the last one
    repeating it; count (int64 [1], optional) = their number.  No host synchronisation (idg_flags_compact_f32).
    Returns (ids, ws) — pass both back to reuse the buffers."""
    _require_device(flags, ids, count, ws)
    if flags.dtype != torch.float32 or not flags.is_contiguous() or flags.dim() != 1:
        raise TypeError("flags_compact_raw: contiguous float32 vector")
    n = int(flags.shape[0])
    if ids is None:
        ids = torch.empty(int(cap), dtype=torch.int64, device=flags.device)
    if ws is None:
        ws = torch.empty(int(lib.idg_flags_compact_workspace_bytes(n)), dtype=torch.uint8, device=flags.device)
    check(lib.idg_flags_compact_f32(_ptr(flags), n, _ptr(ids), int(cap), _ptr(count), _ptr(ws), _stream()),
          "idg_flags_compact_f32")
    return ids, ws


def rows_gather_raw(dst, src, idx):
    """idg_rows_gather_f32: dst[t] = src[idx[t]] (zeros where idx[t] < 0)."""
    _require_device(dst, src, idx)
    check(lib.idg_rows_gather_f32(_ptr(dst), _ptr(src), _ptr(idx), idx.shape[0], src.shape[1], _stream()), "idg_rows_gather_f32")


def rows_chain_add_raw(dst, src, idx, nxt):
    """idg_rows_chain_add_f32: dst[idx[t]] += src[t] + src[nxt[t]] + ... for every chain head t (idx[t] >= 0)."""
    _require_device(dst, src, idx, nxt)
    check(lib.idg_rows_chain_add_f32(_ptr(dst), _ptr(src), _ptr(idx), _ptr(nxt), idx.shape[0], src.shape[1], _stream()),
          "idg_rows_chain_add_f32")


_noise_stream = [0]


def _next_noise_stream():
    """(seed, stream id) of the next perturbation: the seed follows torch's device generator
    (tools.set_seed -> torch.cuda.manual_seed), the stream id counts perturbed layers drawn so far."""
    _noise_stream[0] += 1
    return int(torch.cuda.initial_seed()) & 0xFFFFFFFFFFFFFFFF, _noise_stream[0]


def reset_noise_stream(value=0):
    _noise_stream[0] = int(value)


class _SpMMNoise(torch.autograd.Function):
    """Y = A.X, Y += sign(Y) * normalize(U[0,1)) * eps.  d Y / d X = A (sign has zero gradient)."""

    @staticmethod
    def forward(ctx, X, graph, eps, stream):
        _require_device(X)
        X = _f32c(X, "X")
        ctx.graph = graph
        seed, stream_id = _next_noise_stream() if stream is None else stream
        return spmm_noise_raw(graph, X, eps, seed, stream_id)

    @staticmethod
    def backward(ctx, gY):
        return ctx.graph.T.spmm_raw(gY), None, None, None


def spmm_noise_raw(graph, X, eps, seed, stream_id, out=None, out_rows=None):
    """idg_spmm_noise_f32: one perturbed layer; out_rows: bitmap of the rows to produce."""
    _require_device(X, out, out_rows)
    d = X.shape[1]
    Y = torch.empty((graph.n_rows, d), dtype=torch.float32, device=X.device) if out is None else out
    ws = graph._workspace("spmm", d)
    check(lib.idg_spmm_noise_f32(graph._h, _ptr(X), d, _ptr(Y), d, _ptr(out_rows), d, float(eps), C.c_uint64(seed),
                                 C.c_uint64(stream_id), _ptr(ws), _stream()), "idg_spmm_noise_f32")
    return Y


def spmm_perturbed(graph, X, eps, stream=None):
    """One SimGCL/XSimGCL layer: torch.sparse.mm followed by the in-place noise (models/XSimGCL.py:51-54).
    stream: (seed, stream id) of the noise; default: the next one of the device seed's sequence."""
    return _SpMMNoise.apply(X, graph, float(eps), stream)


def layer_noise_stream(pass_stream, layer):
    """Noise stream of layer `layer` (1-based) of a perturbed K-layer pass drawn as ONE (seed, stream id) —
    what idg_propagate_mean_noise_f32 uses internally, so a layer can be re-produced on its own."""
    seed, sid = pass_stream
    return seed, sid * 64 + int(layer)


def perturb_raw(X, eps, seed, stream_id, out=None, rows=None):
    """idg_perturb_f32: out = X + sign(X) * normalize(u) * eps row by row (the epilogue's perturbation on its own)."""
    _require_device(X, out, rows)
    X = _f32c(X, "X")
    out = torch.empty_like(X) if out is None else out
    check(lib.idg_perturb_f32(_ptr(X), _ptr(out), X.shape[0], X.shape[1], _ptr(rows), float(eps), C.c_uint64(seed),
                              C.c_uint64(stream_id), _stream()), "idg_perturb_f32")
    return out


_compose_views = [False]  # tests: True = assemble the passes from the single-purpose entry points instead


def propagate_views_raw(graph, E0, K, include_layer0, eps, streams, outs, out_rows=None, scratch=None):
    """outs[0] = the clean layer mean of E0, outs[1 + i] = the perturbed one drawn from streams[i] = (seed, stream id)
    (SimGCL's encoder passes, models/SimGCL.py:63-65).  Without layer 0 in the mean and K >= 2 the first product,
    A.E0, is the same in every pass: it is computed ONCE, each view perturbs its own copy (sub-stream 0 of its
    stream) and all passes continue from layer 2 — mean(X1..XK) = propagate_mean(X1, K - 1, include_layer0=True).
    scratch: two [n, d] panels (allocated when None).  out_rows as in propagate_mean_raw."""
    d = E0.shape[1]
    shared = (not include_layer0) and K >= 2 and d in (32, 64, 128, 256, 512)
    if not shared:
        graph.propagate_mean_raw(E0, K, include_layer0, out=outs[0], out_rows=out_rows)
        for out, (seed, sid) in zip(outs[1:], streams):
            graph.propagate_mean_noise_raw(E0, K, include_layer0, eps, seed, sid, out=out, out_rows=out_rows)
        return outs
    if len(streams) <= 2 and not _compose_views[0]:
        # one C call: shared first product, per-view perturbation, and (with out_rows) ONE multi-panel launch for the
        # last layer of all passes — same values as the composition below
        n_views = len(streams)
        ws = _cached_ws(graph._ws, ("views", d, n_views), lambda: lib.idg_propagate_views_workspace_bytes(graph._h, d, n_views),
                        E0.device)
        seeds = (C.c_uint64 * n_views)(*[int(sd) for sd, _ in streams])
        sids = (C.c_uint64 * n_views)(*[int(si) for _, si in streams])
        views = (C.c_void_p * n_views)(*[o.data_ptr() for o in outs[1:]])
        _require_device(E0, out_rows, *outs)
        check(lib.idg_propagate_views_f32(graph._h, _ptr(_f32c(E0, "E0")), int(K), d, float(eps), n_views, seeds, sids,
                                          _ptr(outs[0]), views, _ptr(out_rows), _ptr(ws), _stream()),
              "idg_propagate_views_f32")
        return outs
    T, X1 = scratch if scratch is not None else (torch.empty_like(E0), torch.empty_like(E0))
    graph.spmm_raw(E0, out=T)
    graph.propagate_mean_raw(T, K - 1, True, out=outs[0], out_rows=out_rows)
    for out, (seed, sid) in zip(outs[1:], streams):
        perturb_raw(T, eps, seed, sid * 64, out=X1)  # layer 1 of this view; layers 2..K draw sub-streams 1..K-1
        graph.propagate_mean_noise_raw(X1, K - 1, True, eps, seed, sid, out=out, out_rows=out_rows)
    return outs


class _PropagateViews(torch.autograd.Function):
    """(clean, view_1, ..., view_n): the unperturbed layer mean and n independently perturbed ones.
    Every output has the same Jacobian w.r.t. E0 — (1/cnt) sum_k A^k — so backward adds the incoming
    gradients and propagates ONCE (autograd over separate passes would propagate n + 1 times)."""

    @staticmethod
    def forward(ctx, E0, graph, K, include_layer0, eps, n_views):
        _require_device(E0)
        E0 = _f32c(E0, "E0")
        ctx.graph, ctx.K, ctx.inc = graph, K, include_layer0
        outs = [torch.empty_like(E0) for _ in range(n_views + 1)]
        streams = [_next_noise_stream() for _ in range(n_views)]
        propagate_views_raw(graph, E0, K, include_layer0, eps, streams, outs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        total = None
        for g in grads:
            if g is None:
                continue
            total = g if total is None else total + g
        if total is None:
            return None, None, None, None, None, None
        return ctx.graph.propagate_mean_bwd_raw(total.contiguous(), ctx.K, ctx.inc), None, None, None, None, None


def propagate_views(graph, E0, K, include_layer0, eps, n_views=2):
    """SimGCL's three encoder passes of one step (models/SimGCL.py:63-65) as one differentiable op."""
    return _PropagateViews.apply(E0, graph, int(K), bool(include_layer0), float(eps), int(n_views))


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, graph):
        ctx.graph = graph
        return graph.spmm_raw(X)

    @staticmethod
    def backward(ctx, gY):
        return ctx.graph.T.spmm_raw(gY), None


def spmm(graph, X):
    """Y = A.X — the drop-in for torch.sparse.mm(Graph, X) (models/LightGCN.py:44)."""
    return _SpMM.apply(X, graph)


class _PropagateMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E0, graph, K, include_layer0):
        ctx.graph, ctx.K, ctx.inc = graph, K, include_layer0
        return graph.propagate_mean_raw(E0, K, include_layer0)

    @staticmethod
    def backward(ctx, g):
        if not ctx.graph.symmetric:
            raise RuntimeError("propagate_mean backward needs a symmetric graph; chain spmm() instead")
        return ctx.graph.propagate_mean_bwd_raw(g, ctx.K, ctx.inc), None, None, None


def propagate_mean(graph, E0, K, include_layer0=True):
    """mean_k(A^k E0), k = (0|1)..K — LightGCN.aggregate / SimGCL.aggregate(perturbed=False)."""
    return _PropagateMean.apply(E0, graph, int(K), bool(include_layer0))


# ------------------------------------------------------------------- row normalisation (LightGCN++)
ROWNORM_MAX_WIDTH = 512  # idg_rows_normalize*_f32: 1 <= d <= 512
ROWNORM_EPS = 1e-12  # models/LightGCN_pp.py:83


def _rownorm_args(who, X, norms=None, **panels):
    """The checks of the row-normalisation calls; returns (n, d).  X: contiguous float32 [n, d]; the named panels (None
    allowed) like it; norms: contiguous float32 [n]."""
    if X.dim() != 2:
        raise ValueError("%s: the panel must be [n, d] (got %s)" % (who, tuple(X.shape)))
    n, d = (int(v) for v in X.shape)
    if n < 1 or d < 1 or d > ROWNORM_MAX_WIDTH:
        raise ValueError("%s: %d rows of width %d (at least one row, width 1 .. %d is built)" % (who, n, d, ROWNORM_MAX_WIDTH))
    if X.dtype != torch.float32 or not X.is_contiguous():
        raise TypeError("%s: the panel must be contiguous float32 (got %s, contiguous=%s)" % (who, X.dtype, X.is_contiguous()))
    for name, t in panels.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (n, d)):
            raise TypeError("%s: %s must be a contiguous float32 [%d, %d] tensor" % (who, name, n, d))
    if norms is not None and (norms.dtype != torch.float32 or not norms.is_contiguous() or tuple(norms.shape) != (n,)):
        raise TypeError("%s: norms must be a contiguous float32 [%d] tensor" % (who, n))
    _require_device(X, norms, *panels.values())
    return n, d


def rows_normalize_raw(X, Y=None, norms=None, eps=ROWNORM_EPS):
    """idg_rows_normalize_f32: norms[r] = ||X[r]||_2, Y[r] = X[r] / (norms[r] + eps).  Y may be X (in place).
    Returns (Y, norms)."""
    n, d = _rownorm_args("rows_normalize_raw", X, norms, Y=Y)
    Y = torch.empty_like(X) if Y is None else Y
    norms = torch.empty(n, dtype=torch.float32, device=X.device) if norms is None else norms
    check(lib.idg_rows_normalize_f32(_ptr(X), n, d, float(eps), _ptr(Y), _ptr(norms), _stream()), "idg_rows_normalize_f32")
    return Y, norms


def rows_normalize_bwd_raw(T, Y, norms, G=None, a=0.0, add2=None, out=None, eps=ROWNORM_EPS):
    """idg_rows_normalize_bwd_f32: out[r] = a G[r] + add2[r] + J_r(T[r]), J the backward of the normalisation of row r from the
    Y and norms rows_normalize_raw returned (J(t) = t / eps at a zero row).  G and add2 may each be None; out may be T, G
    or add2.  Returns out."""
    if norms is None or Y is None:
        raise TypeError("rows_normalize_bwd_raw: Y and norms (what rows_normalize_raw returned) are needed")
    n, d = _rownorm_args("rows_normalize_bwd_raw", T, norms, Y=Y, G=G, add2=add2, out=out)
    out = torch.empty_like(T) if out is None else out
    check(lib.idg_rows_normalize_bwd_f32(_ptr(T), _ptr(Y), _ptr(norms), float(eps), _ptr(G), float(a), _ptr(add2), _ptr(out),
                                         n, d, _stream()), "idg_rows_normalize_bwd_f32")
    return out


class _RowsNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, eps):
        Y, norms = rows_normalize_raw(_f32c(X, "X"), eps=eps)
        ctx.save_for_backward(Y, norms)
        ctx.eps = eps
        return Y

    @staticmethod
    def backward(ctx, gY):
        Y, norms = ctx.saved_tensors
        return rows_normalize_bwd_raw(_f32c(gY, "grad"), Y, norms, eps=ctx.eps), None


def rows_normalize(X, eps=ROWNORM_EPS):
    """X / (torch.norm(X, dim=1) + eps)[:, None], differentiable (models/LightGCN_pp.py:83-84)."""
    return _RowsNormalize.apply(X, float(eps))


class _PropagateNormalized(torch.autograd.Function):
    """The encoder of LightGCN++: X_k = A rownorm(X_(k-1)), final = gamma E0 + (1 - gamma) mean(X_1 .. X_K).  Saves the
    normalised inputs N_0 .. N_(K-1) and their norms; the layer outputs themselves are never kept (X_k is normalised in
    place, the running sum rides in the product's epilogue)."""

    @staticmethod
    def forward(ctx, E0, graph, K, gamma):
        E0 = _f32c(E0, "E0")
        _rownorm_args("propagate_normalized", E0)
        if E0.shape[0] != graph.n_cols or graph.n_rows != graph.n_cols:
            raise ValueError("propagate_normalized: E0 must be [%d, d] for this graph, got %s" % (graph.n_cols, tuple(E0.shape)))
        S = torch.empty_like(E0)
        Ns, norms = [], []
        X = E0
        for k in range(1, K + 1):
            # N_(k-1): out of place for the parameters' own panel, in place for a layer output
            N, nrm = rows_normalize_raw(X, Y=None if k == 1 else X)
            Ns.append(N)
            norms.append(nrm)
            last = k == K
            X = None if last else torch.empty_like(E0)
            spmm_ex_raw(graph, N, Y=X, sum_in=None if k == 1 else S, sum_out=S, div=float(K) if last else 1.0)
        final = torch.empty_like(E0)
        lincomb_raw(final, E0, gamma, S, 1.0 - gamma)
        ctx.save_for_backward(*Ns, *norms)
        ctx.graph, ctx.K, ctx.gamma = graph, K, gamma
        return final

    @staticmethod
    def backward(ctx, g):
        K, gamma, At = ctx.K, ctx.gamma, ctx.graph.T
        if At is None:
            raise RuntimeError("propagate_normalized backward needs the transposed graph (Graph(..., symmetric=False) builds it)")
        Ns, norms = ctx.saved_tensors[:K], ctx.saved_tensors[K:]
        g = _f32c(g, "grad")
        c = (1.0 - gamma) / K
        H, T = torch.empty_like(g), torch.empty_like(g)
        lincomb_raw(H, g, c)  # H_K = c g
        for k in range(K, 0, -1):
            At.spmm_raw(H, out=T)
            # H_(k-1) = a g + J_(k-1)(T), written over T
            rows_normalize_bwd_raw(T, Ns[k - 1], norms[k - 1], G=g, a=c if k > 1 else gamma, out=T)
            H, T = T, H
        return H, None, None, None


def propagate_normalized(graph, E0, K, gamma):
    """gamma E0 + (1 - gamma) mean_k(X_k), X_k = A rownorm(X_(k-1)), k = 1..K — LightGCN_pp.aggregate
    (models/LightGCN_pp.py:75-96).  `graph` need not be symmetric: the backward runs on graph.T."""
    K = int(K)
    if K < 1:
        raise ValueError("propagate_normalized: K = %d layers (at least 1)" % K)
    return _PropagateNormalized.apply(E0, graph, K, float(gamma))


# ------------------------------------------------------------------------------------ BPR
_bpr_ws_cache = {}


def bpr_workspace(B, d, device):
    """A private BPR scratch buffer (callers that pipeline batches keep one per in-flight batch)."""
    return torch.empty(int(lib.idg_bpr_workspace_bytes(int(B), int(d))), dtype=torch.uint8, device=device)


def _bpr_ws(B, d, device):
    """Scratch of the fused BPR calls.  One buffer per (batch size, width, device): the forward and
    backward calls of a step (and the side-stream plan) must see the SAME buffer.  Callers that run
    two BPR steps concurrently on different streams need their own workspace (not done here)."""
    return _cached_ws(_bpr_ws_cache, (int(B), int(d), device), lambda: lib.idg_bpr_workspace_bytes(int(B), int(d)), device)


class _BprLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, final_panel, ego_panel, users, pos, neg, num_users, reg_lambda, deterministic):
        _require_device(final_panel, ego_panel, users, pos, neg)
        fin = _f32c(final_panel, "final_panel")
        ego = fin if ego_panel is final_panel else _f32c(ego_panel, "ego_panel")
        users, pos, neg = _i64c(users, "users"), _i64c(pos, "pos"), _i64c(neg, "neg")
        n, d = fin.shape
        B = users.shape[0]
        loss = torch.empty(2, dtype=torch.float32, device=fin.device)
        ws = _bpr_ws(B, d, fin.device)
        check(lib.idg_bpr_forward_f32(_ptr(fin), _ptr(ego), int(num_users), n, _ptr(users), _ptr(pos), _ptr(neg), B, d,
                                      float(reg_lambda), _ptr(loss), _ptr(ws), _stream()), "idg_bpr_forward_f32")
        ctx.save_for_backward(fin, ego, users, pos, neg)
        ctx.meta = (int(num_users), float(reg_lambda), bool(deterministic), ego_panel is final_panel, ws)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_bpr, g_reg):
        fin, ego, users, pos, neg = ctx.saved_tensors
        num_users, reg_lambda, deterministic, same, ws = ctx.meta
        n, d = fin.shape
        B = users.shape[0]
        up = torch.stack([g_bpr.to(torch.float32).reshape(()), g_reg.to(torch.float32).reshape(())]).contiguous()
        g_final = torch.zeros_like(fin)
        g_ego = g_final if same else torch.zeros_like(ego)
        # ws still holds this batch's coefficients: forward and backward of one step are adjacent on the stream
        check(lib.idg_bpr_backward_f32(_ptr(fin), _ptr(ego), num_users, n, _ptr(users), _ptr(pos), _ptr(neg), B, d,
                                       reg_lambda, _ptr(up), _ptr(g_final), _ptr(g_ego), int(deterministic), None,
                                       _ptr(ws), _stream()), "idg_bpr_backward_f32")
        return g_final, (None if same else g_ego), None, None, None, None, None, None


def bpr_loss(final_panel, ego_panel, users, pos, neg, num_users, reg_lambda, deterministic=True):
    """(bpr_loss, reg_lambda * reg_loss) as 0-d tensors, differentiable w.r.t. both panels.

    final_panel / ego_panel: [num_users + num_items, d], users first.  Passing the same
    tensor twice is the MFBPR case (models/MFBPR.py:29-42)."""
    if ego_panel is final_panel:
        out = _BprLossSame.apply(final_panel, users, pos, neg, num_users, reg_lambda, deterministic)
    else:
        out = _BprLoss.apply(final_panel, ego_panel, users, pos, neg, num_users, reg_lambda, deterministic)
    return out


class _BprLossSame(torch.autograd.Function):
    """final == ego: one differentiable input (autograd would otherwise see two aliases)."""

    @staticmethod
    def forward(ctx, panel, users, pos, neg, num_users, reg_lambda, deterministic):
        return _BprLoss.forward(ctx, panel, panel, users, pos, neg, num_users, reg_lambda, deterministic)

    @staticmethod
    def backward(ctx, g_bpr, g_reg):
        g = _BprLoss.backward(ctx, g_bpr, g_reg)
        return g[0], None, None, None, None, None, None


def bpr_touch_rows_raw(users, pos, neg, num_users, bitmap, stream=None, clear_bits=0):
    """Set the bits of the panel rows this batch touches (idg_bpr_touch_rows); bitmap: int32 [ceil(n/32)], zeroed
    by the caller or here when clear_bits = n.  stream: raw handle of the stream to launch on (default: current)."""
    _require_device(users, pos, neg, bitmap)
    _require_ids(users, pos, neg)
    st = _stream() if stream is None else stream
    if clear_bits:
        check(lib.idg_bitmap_clear(_ptr(bitmap), int(clear_bits), st), "idg_bitmap_clear")
    check(lib.idg_bpr_touch_rows(_ptr(users), _ptr(pos), _ptr(neg), users.shape[0], int(num_users), _ptr(bitmap), st),
          "idg_bpr_touch_rows")


def bitmap_clear_raw(bitmap, n_bits, stream=None):
    """idg_bitmap_clear: zero the first n_bits bits of an int32 bitmap tensor."""
    _require_device(bitmap)
    check(lib.idg_bitmap_clear(_ptr(bitmap), int(n_bits), _stream() if stream is None else stream), "idg_bitmap_clear")


def bpr_plan_raw(users, pos, neg, num_users, n, d, ws=None, stream=None):
    """Sort this batch's (row, slot) pairs into the BPR workspace (idg_bpr_plan_f32) on the CURRENT
    stream.  Index-only work: run it on a side stream while the propagation is in flight, then call
    bpr_fused_raw(..., deterministic=2)."""
    _require_device(users, pos, neg)
    _require_ids(users, pos, neg)
    B = users.shape[0]
    ws = _bpr_ws(B, d, users.device) if ws is None else ws
    check(lib.idg_bpr_plan_f32(_ptr(users), _ptr(pos), _ptr(neg), B, int(num_users), int(n), _ptr(ws),
                               _stream() if stream is None else stream), "idg_bpr_plan_f32")


def bpr_fused_raw(final_panel, ego_panel, users, pos, neg, num_users, reg_lambda, g_final, g_ego, loss=None,
                  deterministic=True, touched=None, ws=None):
    """No-autograd form: loss[2] plus gradients accumulated into g_final / g_ego (caller zeroes).
    deterministic: False/0 float atomics, True/1 sort in-call, 2 plan already built (bpr_plan_raw).
    touched: zeroed int32 bitmap [ceil(n/32)]; if given, reached g_final rows are stored + flagged and
    g_final needs no zero-fill (feed the bitmap to Graph.propagate_mean_bwd_raw(mask=...))."""
    _require_device(final_panel, ego_panel, users, pos, neg, g_final, g_ego)
    _require_ids(users, pos, neg)
    n, d = final_panel.shape
    B = users.shape[0]
    loss = torch.empty(2, dtype=torch.float32, device=final_panel.device) if loss is None else loss
    ws = _bpr_ws(B, d, final_panel.device) if ws is None else ws
    check(lib.idg_bpr_fused_f32(_ptr(final_panel), _ptr(ego_panel), int(num_users), n, _ptr(users), _ptr(pos),
                                _ptr(neg), B, d, float(reg_lambda), _ptr(loss), _ptr(g_final), _ptr(g_ego),
                                int(deterministic), _ptr(touched), _ptr(ws), _stream()), "idg_bpr_fused_f32")
    return loss


def bpr_rows_message_floats(B, d):
    """Length (fp32 words) of one rank's gradient-row message (idg_bpr_rows_message_floats)."""
    return int(lib.idg_bpr_rows_message_floats(int(B), int(d)))


def bpr_pack_rows_raw(ws, B, g_final, loss, message, clear=None, clear_bits=0):
    """After bpr_fused_raw(..., deterministic=2, touched=...): this batch's stored g_final rows, the plan's sorted row
    keys (ids and multiplicities) and loss[2] -> `message` (idg_bpr_pack_rows_f32).  clear / clear_bits: a bitmap to zero
    in the same launch (the union bitmap of the coming merge)."""
    _require_device(ws, g_final, loss, message)
    check(lib.idg_bpr_pack_rows_f32(_ptr(ws), int(B), g_final.shape[1], _ptr(g_final), _ptr(loss), _ptr(message),
                                    _ptr(clear), int(clear_bits), _stream()), "idg_bpr_pack_rows_f32")


def bpr_unpack_rows_raw(messages, world, B, ego_panel, reg_lambda, g_final, g_ego, touched, loss, touched_is_clear=False):
    """Merge `world` all-gathered messages in rank order into g_final / g_ego (averaged over ranks), the union
    bitmap `touched` (cleared first) and loss[2] (idg_bpr_unpack_rows_f32)."""
    _require_device(messages, ego_panel, g_final, g_ego, touched, loss)
    n, d = ego_panel.shape
    check(lib.idg_bpr_unpack_rows_f32(_ptr(messages), int(world), int(B), d, n, _ptr(ego_panel), float(reg_lambda),
                                      _ptr(g_final), _ptr(g_ego), _ptr(touched), int(bool(touched_is_clear)), _ptr(loss),
                                      _stream()),
          "idg_bpr_unpack_rows_f32")


def bpr_fwd_bwd_raw(final_panel, ego_panel, users, pos, neg, num_users, reg_lambda, upstream, g_final, g_ego, loss,
                    deterministic=True, ws=None):
    """Forward then backward with the two upstream gradient scalars read from the DEVICE tensor
    `upstream` (the sharded path scales a rank's share of the global batch this way).
    deterministic=2 with `ws` from bpr_plan_raw: the sorted scatter plan is already in the workspace."""
    _require_device(final_panel, ego_panel, users, pos, neg, upstream, g_final, g_ego, loss)
    n, d = final_panel.shape
    B = users.shape[0]
    if ws is None:
        if int(deterministic) == 2:
            raise ValueError("deterministic=2 (planned scatter) needs the workspace bpr_plan_raw filled")
        ws = _bpr_ws(B, d, final_panel.device)
    args = (_ptr(final_panel), _ptr(ego_panel), int(num_users), n, _ptr(users), _ptr(pos), _ptr(neg), B, d,
            float(reg_lambda))
    check(lib.idg_bpr_forward_f32(*args, _ptr(loss), _ptr(ws), _stream()), "idg_bpr_forward_f32")
    check(lib.idg_bpr_backward_f32(*args, _ptr(upstream), _ptr(g_final), _ptr(g_ego), int(deterministic), None,
                                   _ptr(ws), _stream()), "idg_bpr_backward_f32")
    return loss


# ----------------------------------------------------------------------------------- thin dense layer
_wgrad_ws = {}


def linear_wgrad_raw(X, G, out=None, accumulate=False):
    """idg_linear_wgrad_f32: out[d1, d2] (+)= X^T . G for tall X [n, d1], G [n, d2]."""
    _require_device(X, G, out)
    X, G = _f32c(X, "X"), _f32c(G, "G")
    n, d1 = X.shape
    d2 = G.shape[1]
    if G.shape[0] != n:
        raise ValueError("linear_wgrad_raw: X and G must have the same number of rows")
    if out is None:
        out = torch.empty((d1, d2), dtype=torch.float32, device=X.device)
    ws = _cached_ws(_wgrad_ws, (n, d1, d2, X.device), lambda: lib.idg_linear_wgrad_workspace_bytes(n, d1, d2), X.device)
    check(lib.idg_linear_wgrad_f32(_ptr(X), d1, _ptr(G), d2, n, d1, d2, _ptr(out), int(bool(accumulate)), _ptr(ws), _stream()),
          "idg_linear_wgrad_f32")
    return out


_colsum_ws = {}


def colsum_raw(X, out=None, accumulate=False):
    """out[f] (+)= sum_r X[r, f] (idg_colsum_f32: row slices summed in slice order, deterministic)."""
    _require_device(X, out)
    X = _f32c(X, "X")
    n, d = X.shape
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=X.device)
    ws = _cached_ws(_colsum_ws, (d, X.device), lambda: lib.idg_colsum_workspace_bytes(d), X.device)
    check(lib.idg_colsum_f32(_ptr(X), d, n, d, _ptr(out), int(bool(accumulate)), _ptr(ws), _stream()), "idg_colsum_f32")
    return out


class _TallLinear(torch.autograd.Function):
    """Y = X @ W for X [n, d1] with n >> d1, d2 (NGCF's per-layer transforms).  Forward and the input gradient are
    ordinary small (NN) GEMMs; the weight gradient X^T @ gY is all reduction and goes to idg_linear_wgrad_f32."""

    @staticmethod
    def forward(ctx, X, W):
        ctx.save_for_backward(X, W)
        return torch.matmul(X, W)

    @staticmethod
    def backward(ctx, gY):
        X, W = ctx.saved_tensors
        # gY @ W^T as an NN GEMM on a transposed copy of the small weight: the NT form makes the BLAS library pick
        # a 200 us kernel for [n, 64] x [64, 64] (measured; the NN form of the same product takes 16 us)
        gX = torch.matmul(gY, W.t().contiguous()) if ctx.needs_input_grad[0] else None
        gW = linear_wgrad_raw(X, gY.contiguous()) if ctx.needs_input_grad[1] else None
        return gX, gW


def tall_linear(X, W):
    """torch.matmul(X, W) with a weight gradient sized for n >> d (models/NGCF.py:91-99)."""
    return _TallLinear.apply(X, W)


class _NgcfTransform(torch.autograd.Function):
    """S = side @ W1 + (ego * side) @ W2 on the fp32 matrix cores in one pass over the rows (idg_ngcf_transform_f32);
    backward: input gradients by idg_ngcf_transform_bwd_f32, weight gradients by idg_linear_wgrad_f32."""

    @staticmethod
    def forward(ctx, side, ego, W1, W2):
        _require_device(side, ego, W1, W2)
        side, ego, W1, W2 = _f32c(side, "side"), _f32c(ego, "ego"), _f32c(W1, "W1"), _f32c(W2, "W2")
        n, d1 = side.shape
        d2 = W1.shape[1]
        S = torch.empty((n, d2), dtype=torch.float32, device=side.device)
        need_w = ctx.needs_input_grad[3]
        BI = torch.empty_like(side) if need_w else None
        check(lib.idg_ngcf_transform_f32(_ptr(side), _ptr(ego), _ptr(W1), _ptr(W2), n, d1, d2, _ptr(S), _ptr(BI), _stream()),
              "idg_ngcf_transform_f32")
        ctx.save_for_backward(side, ego, W1, W2, BI if need_w else side)
        ctx.has_bi = need_w
        return S

    @staticmethod
    def backward(ctx, gS):
        side, ego, W1, W2, BI = ctx.saved_tensors
        gS = _f32c(gS, "gS")
        n, d1 = side.shape
        d2 = W1.shape[1]
        g_side = g_ego = gW1 = gW2 = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g_side, g_ego = torch.empty_like(side), torch.empty_like(side)
            check(lib.idg_ngcf_transform_bwd_f32(_ptr(gS), _ptr(side), _ptr(ego), _ptr(W1), _ptr(W2), n, d1, d2, _ptr(g_side),
                                                 _ptr(g_ego), _stream()), "idg_ngcf_transform_bwd_f32")
        if ctx.needs_input_grad[2]:
            gW1 = linear_wgrad_raw(side, gS)
        if ctx.needs_input_grad[3]:
            gW2 = linear_wgrad_raw(BI if ctx.has_bi else ego * side, gS)
        return g_side, g_ego, gW1, gW2


def ngcf_transform(side, ego, W1, W2):
    """torch.matmul(side, W1) + torch.matmul(ego * side, W2) (models/NGCF.py:88-99, biases left to ngcf_layer_tail).
    MFMA kernel when the widths allow it (d1 % 64 == 0 and d2 % 64 == 0), the two thin GEMMs otherwise."""
    d1, d2 = W1.shape
    if d1 % 64 == 0 and d2 % 64 == 0 and side.is_cuda and os.environ.get("IDG_NGCF_MFMA", "1") != "0":
        return _NgcfTransform.apply(side, ego, W1, W2)
    return tall_linear(side, W1) + tall_linear(torch.mul(ego, side), W2)


class _NgcfTail(torch.autograd.Function):
    """(E, N) = NGCF's layer tail of (S1, S2, b1, b2): leaky_relu((S1 + b1) + (S2 + b2)) -> dropout -> (itself,
    its row-normalised copy) in one kernel; backward in one kernel + the bias column sums."""

    @staticmethod
    def forward(ctx, S1, S2, b1, b2, slope, p, stream):
        _require_device(S1, S2, b1, b2)
        S1, S2 = _f32c(S1, "S1"), (None if S2 is None else _f32c(S2, "S2"))
        n, d = S1.shape
        E, N = torch.empty_like(S1), torch.empty_like(S1)
        seed, sid = stream
        check(lib.idg_ngcf_tail_f32(_ptr(S1), _ptr(S2), _ptr(_f32c(b1.reshape(-1), "b1")), _ptr(_f32c(b2.reshape(-1), "b2")), n, d,
                                    float(slope), float(p), C.c_uint64(seed), C.c_uint64(sid), _ptr(E), _ptr(N), _stream()),
              "idg_ngcf_tail_f32")
        ctx.save_for_backward(E)
        ctx.args = (float(slope), float(p), seed, sid, b1.shape, b2.shape)
        return E, N

    @staticmethod
    def backward(ctx, gE, gN):
        (E,) = ctx.saved_tensors
        slope, p, seed, sid, shape1, shape2 = ctx.args
        n, d = E.shape
        gE = None if gE is None else _f32c(gE, "gE")
        gN = None if gN is None else _f32c(gN, "gN")
        gT = torch.empty_like(E)
        check(lib.idg_ngcf_tail_bwd_f32(_ptr(E), _ptr(gE), _ptr(gN), n, d, slope, p, C.c_uint64(seed), C.c_uint64(sid),
                                        _ptr(gT), _stream()), "idg_ngcf_tail_bwd_f32")
        gb = colsum_raw(gT)  # the two bias rows receive the same gradient: the column sums of gT
        return gT, (gT if ctx.needs_input_grad[1] else None), gb.reshape(shape1), gb.reshape(shape2), None, None, None


def ngcf_layer_tail(S1, S2, b1, b2, negative_slope=0.2, p=0.0, stream=None):
    """(next ego, its L2-normalised copy) of one NGCF layer from the two transformed panels (models/NGCF.py:95-108);
    S2 = None: S1 already holds their sum (ngcf_transform).
    stream: (seed, stream id) of the dropout mask; default: the next one of the device seed's sequence."""
    return _NgcfTail.apply(S1, S2, b1, b2, negative_slope, p, _next_noise_stream() if stream is None else stream)


# ----------------------------------------------------------------------------------- LR-GCCF's linear layer
_gccf_ws = {}


def gccf_layer_fwd_raw(side, W, b, p, seed, stream_id, E, lde=None, slot=0):
    """idg_gccf_layer_fwd_f32: E[r, 0:64] = keep * (side[r] . W + b), written `slot` floats into each row of E with leading
    dimension lde (default: E's own width)."""
    _require_device(side, W, b, E)
    n, d = side.shape
    check(lib.idg_gccf_layer_fwd_f32(_ptr(side), _ptr(W), _ptr(b), n, d, float(p), C.c_uint64(seed), C.c_uint64(stream_id),
                                     E.data_ptr() + 4 * int(slot), int(E.shape[1] if lde is None else lde), _stream()),
          "idg_gccf_layer_fwd_f32")
    return E


def gccf_layer_bwd_raw(gE, gN, ldgn, gn_rows, side, W, p, seed, stream_id, g_side, w_grads, gn_slot=0):
    """idg_gccf_layer_bwd_f32: gT = keep * (gE + gN at the rows of the bitmap gn_rows); g_side = gT . W^T;
    w_grads = [side^T . gT | column sums of gT].  gN is read `gn_slot` floats into each row, leading dimension ldgn."""
    _require_device(gE, gN, gn_rows, side, W, g_side, w_grads)
    n, d = side.shape
    ws = _cached_ws(_gccf_ws, (d, side.device), lambda: max(int(lib.idg_gccf_layer_bwd_workspace_bytes(d)), 16), side.device)
    check(lib.idg_gccf_layer_bwd_f32(_ptr(gE), None if gN is None else gN.data_ptr() + 4 * int(gn_slot), int(ldgn), _ptr(gn_rows),
                                     _ptr(side), _ptr(W), n, d, float(p), C.c_uint64(seed), C.c_uint64(stream_id), _ptr(g_side),
                                     _ptr(w_grads), _ptr(ws), _stream()), "idg_gccf_layer_bwd_f32")
    return g_side, w_grads


class _GccfLayer(torch.autograd.Function):
    """E = dropout(side @ W + b) at d = 64 in one kernel per direction (csrc/idg_gccf.hip).  The backward needs no saved
    activation: the mask is regenerated from (seed, stream id), and the layer is linear in between."""

    @staticmethod
    def forward(ctx, side, W, b, p, stream):
        seed, sid = stream
        E = torch.empty_like(side)
        gccf_layer_fwd_raw(side, W, b.reshape(-1), p, seed, sid, E)
        ctx.save_for_backward(side, W)
        ctx.args = (float(p), seed, sid, b.shape)
        return E

    @staticmethod
    def backward(ctx, gE):
        side, W = ctx.saved_tensors
        p, seed, sid, b_shape = ctx.args
        d = W.shape[0]
        g_side = torch.empty_like(side)
        w_grads = torch.empty(d * d + d, dtype=torch.float32, device=side.device)
        gccf_layer_bwd_raw(_f32c(gE, "gE"), None, d, None, side, W, p, seed, sid, g_side, w_grads)
        return g_side, w_grads[:d * d].view(d, d), w_grads[d * d:].view(b_shape), None, None


def gccf_layer(side, W, b, p, stream=None):
    """One LR-GCCF layer after the sparse product: nn.Dropout(p)(torch.matmul(side, W) + b) (Chen et al., AAAI'20).
    side [n, d1], W [d1, d2], b [1, d2] or [d2].  d1 = d2 = 64: idg_gccf_layer_fwd_f32 / idg_gccf_layer_bwd_f32; any other
    width: tall_linear and ngcf_layer_tail with slope 1 and a zero second bias, whose first output is exactly
    dropout(S + b).  stream: (seed, stream id) of the dropout mask; default: the next one of the device seed's sequence."""
    for t, name in ((side, "side"), (W, "W"), (b, "b")):
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    if side.dim() != 2 or W.dim() != 2:
        raise ValueError("gccf_layer: side must be [n, d] and W [d, d2], got %s and %s" % (tuple(side.shape), tuple(W.shape)))
    if side.shape[1] != W.shape[0] or b.numel() != W.shape[1]:
        raise ValueError("gccf_layer: side %s, W %s and b %s do not fit (side [n, d], W [d, d2], b [1, d2])"
                         % (tuple(side.shape), tuple(W.shape), tuple(b.shape)))
    if side.shape[0] == 0:
        raise ValueError("gccf_layer: side has 0 rows")
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("gccf_layer: drop probability p = %g outside [0, 1)" % float(p))
    _require_device(side, W, b)
    stream = _next_noise_stream() if stream is None else stream
    if tuple(W.shape) == (64, 64):
        return _GccfLayer.apply(_f32c(side, "side"), _f32c(W, "W"), _f32c(b, "b"), float(p), stream)
    return ngcf_layer_tail(tall_linear(side, W), None, b, torch.zeros_like(b), 1.0, float(p), stream)[0]


# ----------------------------------------------------------------------------------- GCMC's two-transform layer
GCMC_SLOPE = 0.2  # nn.LeakyReLU(negative_slope=0.2) (models/GCMC.py:80)
_gcmc_ws = {}


def gcmc_layer_fwd_raw(side, Wg, bg, Wm, bm, p, seed, stream_id, T, N, ldn=None, slot=0, slope=GCMC_SLOPE):
    """idg_gcmc_layer_fwd_f32: T = keep * (leaky_relu(side . Wg + bg) . Wm + bm) contiguous [n, 64]; N = T / max(|T|, 1e-12)
    written `slot` floats into each row of N with leading dimension ldn (default: N's own width)."""
    _require_device(side, Wg, bg, Wm, bm, T, N)
    n, d = side.shape
    check(lib.idg_gcmc_layer_fwd_f32(_ptr(side), _ptr(Wg), _ptr(bg), _ptr(Wm), _ptr(bm), n, d, float(slope), float(p),
                                     C.c_uint64(seed), C.c_uint64(stream_id), _ptr(T), N.data_ptr() + 4 * int(slot),
                                     int(N.shape[1] if ldn is None else ldn), _stream()), "idg_gcmc_layer_fwd_f32")
    return T, N


def gcmc_layer_bwd_raw(T, gE, gN, ldgn, gn_rows, side, Wg, bg, Wm, p, seed, stream_id, g_side, w_grads, gn_slot=0,
                       slope=GCMC_SLOPE):
    """idg_gcmc_layer_bwd_f32: gM = keep * (gE + J_normalize(T)^T gN at the rows of the bitmap gn_rows), then the layer's
    backward with H and A recomputed from side; g_side [n, 64]; w_grads = [gWg | gbg | gWm | gbm].  gN is read `gn_slot`
    floats into each row, leading dimension ldgn."""
    _require_device(T, gE, gN, gn_rows, side, Wg, bg, Wm, g_side, w_grads)
    n, d = side.shape
    ws = _cached_ws(_gcmc_ws, (d, side.device), lambda: max(int(lib.idg_gcmc_layer_bwd_workspace_bytes(d)), 16), side.device)
    check(lib.idg_gcmc_layer_bwd_f32(_ptr(T), _ptr(gE), None if gN is None else gN.data_ptr() + 4 * int(gn_slot), int(ldgn),
                                     _ptr(gn_rows), _ptr(side), _ptr(Wg), _ptr(bg), _ptr(Wm), n, d, float(slope), float(p),
                                     C.c_uint64(seed), C.c_uint64(stream_id), _ptr(g_side), _ptr(w_grads), _ptr(ws), _stream()),
          "idg_gcmc_layer_bwd_f32")
    return g_side, w_grads


class _GcmcLayer(torch.autograd.Function):
    """(T, N) of one GCMC layer at d = 64 in one kernel per direction (csrc/idg_gcmc.hip).  The backward reads T and side:
    H and A are recomputed, the mask regenerated from (seed, stream id)."""

    @staticmethod
    def forward(ctx, side, Wg, bg, Wm, bm, p, stream):
        seed, sid = stream
        T, N = torch.empty_like(side), torch.empty_like(side)
        gcmc_layer_fwd_raw(side, Wg, bg.reshape(-1), Wm, bm.reshape(-1), p, seed, sid, T, N)
        ctx.save_for_backward(side, Wg, bg, Wm, T)
        ctx.args = (float(p), seed, sid, bg.shape, bm.shape)
        return T, N

    @staticmethod
    def backward(ctx, gT, gN):
        side, Wg, bg, Wm, T = ctx.saved_tensors
        p, seed, sid, bg_shape, bm_shape = ctx.args
        d = Wg.shape[0]
        g_side = torch.empty_like(side)
        w_grads = torch.empty(2 * (d * d + d), dtype=torch.float32, device=side.device)
        gcmc_layer_bwd_raw(T, None if gT is None else _f32c(gT, "gT"), None if gN is None else _f32c(gN, "gN"), d, None, side, Wg,
                           bg.reshape(-1), Wm, p, seed, sid, g_side, w_grads)
        h = d * d + d
        return (g_side, w_grads[:d * d].view(d, d), w_grads[d * d:h].view(bg_shape), w_grads[h:h + d * d].view(d, d),
                w_grads[h + d * d:].view(bm_shape), None, None)


def gcmc_layer(side, Wg, bg, Wm, bm, p, stream=None):
    """One GCMC layer after the sparse product (models/GCMC.py:77-88): M = leaky_relu(side @ Wg + bg, 0.2) @ Wm + bm,
    T = nn.Dropout(p)(M) (the next layer's input), N = normalize(T) (what is concatenated).  Returns (T, N).
    side [n, d1], Wg [d1, d2], Wm [d2, d3], biases [1, .] or [.].  Both matrices [64, 64]: idg_gcmc_layer_fwd_f32 /
    idg_gcmc_layer_bwd_f32; any other width, and rectangular layers: tall_linear and ngcf_layer_tail twice — slope 0.2 without
    a mask for the activation, then slope 1 with the mask, whose outputs are exactly (dropout(M), its normalised copy).
    stream: (seed, stream id) of the dropout mask; default: the next one of the device seed's sequence."""
    for t, name in ((side, "side"), (Wg, "Wg"), (bg, "bg"), (Wm, "Wm"), (bm, "bm")):
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    if side.dim() != 2 or Wg.dim() != 2 or Wm.dim() != 2:
        raise ValueError("gcmc_layer: side must be [n, d], Wg [d, d2] and Wm [d2, d3], got %s, %s and %s"
                         % (tuple(side.shape), tuple(Wg.shape), tuple(Wm.shape)))
    if side.shape[1] != Wg.shape[0] or bg.numel() != Wg.shape[1] or Wm.shape[0] != Wg.shape[1] or bm.numel() != Wm.shape[1]:
        raise ValueError("gcmc_layer: side %s, Wg %s, bg %s, Wm %s and bm %s do not fit (side [n, d], Wg [d, d2], bg [1, d2], "
                         "Wm [d2, d3], bm [1, d3])" % tuple(tuple(t.shape) for t in (side, Wg, bg, Wm, bm)))
    if side.shape[0] == 0:
        raise ValueError("gcmc_layer: side has 0 rows")
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("gcmc_layer: drop probability p = %g outside [0, 1)" % float(p))
    _require_device(side, Wg, bg, Wm, bm)
    stream = _next_noise_stream() if stream is None else stream
    if tuple(Wg.shape) == (64, 64) and tuple(Wm.shape) == (64, 64):
        return _GcmcLayer.apply(_f32c(side, "side"), _f32c(Wg, "Wg"), _f32c(bg, "bg"), _f32c(Wm, "Wm"), _f32c(bm, "bm"), float(p),
                                stream)
    A = ngcf_layer_tail(tall_linear(side, Wg), None, bg, torch.zeros_like(bg), GCMC_SLOPE, 0.0, stream)[0]
    return ngcf_layer_tail(tall_linear(A, Wm), None, bm, torch.zeros_like(bm), 1.0, float(p), stream)


# ----------------------------------------------------------------------------------- IMP-GCN's groups
IMPGCN_SLOPE = 0.01  # nn.LeakyReLU() (models/IMPGCN.py:35)
IMPGCN_DROP = 0.4    # nn.Dropout(p=0.4), hard-coded (models/IMPGCN.py:36)
GROUP_MAX = 8        # a membership is one byte


class GroupCsr:
    """A plain device CSR (indptr int64, indices int32 ascending per row, values fp32; square) for idg_grouped_spmm_f32, with
    the schedule of its rows longer than one chunk (built once, on the host) and, optionally, the ops.Graph handle of the
    same matrix, through which widths other than 64 are composed.  The host arrays are checked here — every index inside
    0 .. n - 1, indptr monotone from 0 to nnz: the kernel trusts them."""

    def __init__(self, indptr, indices, values, n, device, graph=None, schedule=True):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.float32)
        n = int(n)
        if indptr.shape != (n + 1,) or indices.shape != values.shape or indices.ndim != 1:
            raise ValueError("GroupCsr: indptr must be [n + 1] and indices / values [nnz] (got %s, %s, %s for n = %d)"
                             % (indptr.shape, indices.shape, values.shape, n))
        lens = np.diff(indptr)
        if n < 1 or indptr[0] != 0 or indptr[-1] != indices.shape[0] or (lens < 0).any():
            raise ValueError("GroupCsr: indptr must rise from 0 to nnz = %d over n >= 1 rows" % indices.shape[0])
        if indices.shape[0] and (indices.min() < 0 or indices.max() >= n):
            raise ValueError("GroupCsr: a column index lies outside 0 .. %d (the matrix is square)" % (n - 1))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("idgrec_amd operators run on MI355X only: GroupCsr needs a cuda(HIP) device, got %s" % dev)
        self.n, self.nnz, self.device, self.graph = n, int(indices.shape[0]), dev, graph
        self.indptr = torch.from_numpy(indptr).to(dev)
        self.indices = torch.from_numpy(indices).to(dev)
        self.values = torch.from_numpy(values).to(dev)
        chunk = int(lib.idg_grouped_spmm_chunk())
        long_rows = np.nonzero(lens > chunk)[0].astype(np.int32) if schedule else np.zeros(0, dtype=np.int32)
        chunk0 = np.concatenate([[0], np.cumsum((lens[long_rows] + chunk - 1) // chunk)]).astype(np.int32)
        self.n_long, self.n_chunks = int(long_rows.shape[0]), int(chunk0[-1])
        self.long_rows = torch.from_numpy(long_rows).to(dev) if self.n_long else None
        self.long_chunk0 = torch.from_numpy(chunk0).to(dev) if self.n_long else None
        self._ws = {}

    @classmethod
    def from_scipy(cls, mat, device, graph=None, schedule=True):
        m = mat.tocsr().astype(np.float32)
        m.sort_indices()
        if m.shape[0] != m.shape[1]:
            raise ValueError("GroupCsr: the matrix must be square, got %s" % (m.shape,))
        return cls(m.indptr, m.indices, m.data, m.shape[0], device, graph=graph, schedule=schedule)

    def workspace(self, G):
        if not self.n_long:
            return None
        return _cached_ws(self._ws, G, lambda: lib.idg_grouped_spmm_workspace_bytes(self.n_chunks, G), self.device)


def _check_groups(who, G):
    if int(G) != G or not 1 <= int(G) <= GROUP_MAX:
        raise ValueError("%s: G = %s outside 1 .. %d (a membership is one byte)" % (who, G, GROUP_MAX))
    return int(G)


def _check_member(who, member, n):
    if member.dtype != torch.uint8:
        raise TypeError("%s: member must be uint8, one byte per node (got %s)" % (who, member.dtype))
    if tuple(member.shape) != (n,) or not member.is_contiguous():
        raise ValueError("%s: member must be a contiguous [%d] vector, got %s" % (who, n, tuple(member.shape)))


def group_assign_raw(ego, side, W_fc, b_fc, W_grp, b_grp, num_users, p, seed, stream_fc, stream_grp, member=None, scores_out=None,
                     slope=IMPGCN_SLOPE):
    """idg_group_assign_f32: member[r] = the bitmask of the groups whose masked score is the row's maximum (user rows), every
    group (rows >= num_users).  ego, side [n, 64]; W_fc [64, 64], W_grp [G, 64] in nn.Linear's [out, in] layout.  The two
    masks are the published function of (seed, stream_fc, row, feature) and (seed, stream_grp, row, g).  scores_out [n, G]
    (optional) receives the masked scores as compared.  Returns member (uint8 [n])."""
    who = "group_assign_raw"
    for t, name in ((ego, "ego"), (side, "side"), (W_fc, "W_fc"), (b_fc, "b_fc"), (W_grp, "W_grp"), (b_grp, "b_grp"), (scores_out, "scores_out")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32 (got %s)" % (who, name, t.dtype))
    if ego.dim() != 2 or ego.shape[1] != 64 or ego.shape != side.shape or ego.shape[0] == 0:
        raise ValueError("%s: ego and side must both be [n >= 1, 64], got %s and %s" % (who, tuple(ego.shape), tuple(side.shape)))
    n = int(ego.shape[0])
    if tuple(W_fc.shape) != (64, 64) or b_fc.numel() != 64 or W_grp.dim() != 2 or W_grp.shape[1] != 64 or b_grp.numel() != W_grp.shape[0]:
        raise ValueError("%s: W_fc %s, b_fc %s, W_grp %s and b_grp %s do not fit ([64, 64], [64], [G, 64], [G])"
                         % (who, tuple(W_fc.shape), tuple(b_fc.shape), tuple(W_grp.shape), tuple(b_grp.shape)))
    G = _check_groups(who, W_grp.shape[0])
    if not 0 <= int(num_users) <= n:
        raise ValueError("%s: num_users = %d outside 0 .. n = %d" % (who, num_users, n))
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("%s: drop probability p = %g outside [0, 1)" % (who, float(p)))
    if member is None:
        member = torch.empty(n, dtype=torch.uint8, device=ego.device)
    _check_member(who, member, n)
    if scores_out is not None and (tuple(scores_out.shape) != (n, G) or not scores_out.is_contiguous()):
        raise ValueError("%s: scores_out must be a contiguous [%d, %d] panel, got %s" % (who, n, G, tuple(scores_out.shape)))
    _require_device(ego, side, W_fc, b_fc, W_grp, b_grp, member, scores_out)
    check(lib.idg_group_assign_f32(_ptr(_f32c(ego, "ego")), _ptr(_f32c(side, "side")), _ptr(_f32c(W_fc, "W_fc")), _ptr(_f32c(b_fc, "b_fc")),
                                   _ptr(_f32c(W_grp, "W_grp")), _ptr(_f32c(b_grp, "b_grp")), n, 64, G, int(num_users), float(slope),
                                   float(p), C.c_uint64(seed), C.c_uint64(stream_fc), C.c_uint64(stream_grp), _ptr(member),
                                   _ptr(scores_out), _stream()), "idg_group_assign_f32")
    return member


def grouped_spmm_raw(csr, member, X, G, V=None, Y=None, S=None, S_in=None, x_rows=None, v_rows=None):
    """idg_grouped_spmm_f32 on a GroupCsr: t_g[r] = sum_k values[k] [g in m(col_k)] (X_g[col_k] + V[col_k]) for g in m(r).
    X: [n, 64] (shared by the groups) or [G, n, 64]; V: [n, 64] or None.  Y [G, n, 64] receives t_g at the rows with g in m(r)
    (the others are NOT written), S [n, 64] receives (S_in or 0) + sum_g t_g; at least one of them; S_in may be S.
    x_rows (shared X only) / v_rows: int32 bitmaps of the live rows of X / V — the others count as zero and are not read."""
    who = "grouped_spmm_raw"
    if not isinstance(csr, GroupCsr):
        raise TypeError("%s: csr must be an ops.GroupCsr (got %s)" % (who, type(csr).__name__))
    G, n = _check_groups(who, G), csr.n
    for t, name in ((X, "X"), (V, "V"), (Y, "Y"), (S, "S"), (S_in, "S_in")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32 (got %s)" % (who, name, t.dtype))
    for t, name in ((x_rows, "x_rows"), (v_rows, "v_rows")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < (n + 31) // 32 or not t.is_contiguous()):
            raise TypeError("%s: %s must be a contiguous int32 bitmap of >= %d words" % (who, name, (n + 31) // 32))
    _check_member(who, member, n)
    grouped = X.dim() == 3
    if tuple(X.shape) != ((G, n, 64) if grouped else (n, 64)) or not X.is_contiguous():
        raise ValueError("%s: X must be a contiguous [%d, 64] or [%d, %d, 64] panel, got %s" % (who, n, G, n, tuple(X.shape)))
    for t, name in ((V, "V"), (S, "S"), (S_in, "S_in")):
        if t is not None and (tuple(t.shape) != (n, 64) or not t.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous [%d, 64] panel, got %s" % (who, name, n, tuple(t.shape)))
    if Y is not None and (tuple(Y.shape) != (G, n, 64) or not Y.is_contiguous()):
        raise ValueError("%s: Y must be a contiguous [%d, %d, 64] panel, got %s" % (who, G, n, tuple(Y.shape)))
    if Y is None and S is None:
        raise ValueError("%s: at least one of Y and S must be given" % who)
    if S_in is not None and S is None:
        raise ValueError("%s: S_in without S" % who)
    if x_rows is not None and grouped:
        raise ValueError("%s: x_rows names the live rows of a SHARED X only" % who)
    if v_rows is not None and V is None:
        raise ValueError("%s: v_rows without V" % who)
    _require_device(member, X, V, Y, S, S_in, x_rows, v_rows)
    check(lib.idg_grouped_spmm_f32(n, csr.nnz, _ptr(csr.indptr), _ptr(csr.indices), _ptr(csr.values), 64, G, _ptr(member), _ptr(X),
                                   n * 64 if grouped else 0, _ptr(x_rows), _ptr(V), _ptr(v_rows), _ptr(Y), n * 64, _ptr(S_in), _ptr(S),
                                   _ptr(csr.long_rows), _ptr(csr.long_chunk0), csr.n_long, csr.n_chunks, _ptr(csr.workspace(G)),
                                   _stream()), "idg_grouped_spmm_f32")
    return Y, S


def group_grad_raw(S, a, gF, b, GE, rows, out):
    """idg_group_grad_f32: out[r] = a * S[r] + (r flagged in rows ? b * gF[r] + GE[r] : 0); S may be None (zero) or out."""
    _require_device(S, gF, GE, rows, out)
    n, d = out.shape
    check(lib.idg_group_grad_f32(_ptr(S), float(a), _ptr(gF), float(b), _ptr(GE), _ptr(rows), n, d, _ptr(out), _stream()),
          "idg_group_grad_f32")
    return out


class _GroupedPropagate(torch.autograd.Function):
    """[S_1 .. S_P] (or their sum) of P chained grouped products at d = 64, S_l = sum_g X_g^l, X_g^l = A_g X_g^(l-1), X_g^0 =
    E0.  Linear in E0 for a fixed membership and A_g symmetric, so the backward is the Horner chain through the same kernel:
    H_g <- A_g gS_P, H_g <- A_g (gS_l + H_g) for l = P-1 .. 1, then sum_g H_g — no forward panel is kept."""

    @staticmethod
    def forward(ctx, E0, csr, member, P, G, summed):
        n = csr.n
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=E0.device)  # noqa: E731
        ctx.csr, ctx.member, ctx.P, ctx.G, ctx.summed = csr, member, P, G, summed
        X, outs, S = E0, [], None
        ping = [new(G, n, 64) if P > 2 else None, new(G, n, 64) if P > 1 else None]  # X^l goes to ping[l % 2]
        for l in range(1, P + 1):
            Y = ping[l % 2] if l < P else None
            if summed:
                S_in, S = S, (new(n, 64) if S is None else S)
            else:
                S_in, S = None, new(n, 64)
                outs.append(S)
            grouped_spmm_raw(csr, member, X, G, Y=Y, S=S, S_in=S_in)
            X = Y
        return S if summed else tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        csr, member, P, G = ctx.csr, ctx.member, ctx.P, ctx.G
        n = csr.n
        gs = [grads[0]] * P if ctx.summed else list(grads)
        gs = [None if g is None else _f32c(g, "grad") for g in gs]
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=member.device)  # noqa: E731
        H, ping, out = None, [None, None], None
        for l in range(P, 0, -1):
            g = gs[l - 1]
            if H is None and g is None:
                continue
            if l > 1:
                if ping[l % 2] is None:
                    ping[l % 2] = new(G, n, 64)
                Y, S = ping[l % 2], None
            else:
                Y, S = None, new(n, 64)
                out = S
            if H is None:
                grouped_spmm_raw(csr, member, g, G, Y=Y, S=S)
            else:
                grouped_spmm_raw(csr, member, H, G, V=g, Y=Y, S=S)
            H = Y
        if out is None:
            out = torch.zeros((n, 64), dtype=torch.float32, device=member.device)
        return out, None, None, None, None, None


def grouped_propagate(csr, E0, member, n_products, groups, summed=False):
    """IMP-GCN's propagation (models/IMPGCN.py:66-81) for a fixed membership: the list [S_1 .. S_P], P = n_products =
    GCN_layer - 1, of the group sums S_l = sum_g (D_g A D_g)^l E0 (groups ascending), or their sum when `summed`.
    Differentiable in E0.  d = 64: idg_grouped_spmm_f32 in both directions, one walk of the adjacency per product for all
    groups; any other width: per group, rows masked in torch, ops.spmm on csr.graph (the ops.Graph of the same matrix),
    masked again."""
    who = "grouped_propagate"
    if not isinstance(csr, GroupCsr):
        raise TypeError("%s: csr must be an ops.GroupCsr (got %s)" % (who, type(csr).__name__))
    if E0.dtype != torch.float32:
        raise TypeError("%s: E0 must be float32 (got %s)" % (who, E0.dtype))
    if E0.dim() != 2 or E0.shape[0] != csr.n:
        raise ValueError("%s: E0 must be [%d, d], got %s" % (who, csr.n, tuple(E0.shape)))
    G = _check_groups(who, groups)
    P = int(n_products)
    if P < 0:
        raise ValueError("%s: n_products = %d below 0" % (who, P))
    _check_member(who, member, csr.n)
    _require_device(E0, member)
    if P == 0:
        return torch.zeros_like(E0) if summed else []
    if E0.shape[1] == 64:
        out = _GroupedPropagate.apply(_f32c(E0, "E0"), csr, member, P, G, bool(summed))
        return out if summed else list(out)
    if csr.graph is None:
        raise ValueError("%s: a width other than 64 (got %d) is composed through csr.graph, which this GroupCsr was made without"
                         % (who, E0.shape[1]))
    sums = [None] * P
    for g in range(G):
        mask = ((member >> g) & 1).to(torch.float32)[:, None]
        X = E0
        for l in range(P):
            X = mask * spmm(csr.graph, mask * X)
            sums[l] = X if sums[l] is None else sums[l] + X
    if summed:
        total = sums[0]
        for s in sums[1:]:
            total = total + s
        return total
    return sums


# ----------------------------------------------------------------------------------- BIGCF's intent layer
_intent_ws = {}


def intent_noise_raw(out, seed, stream_id, base_row=0):
    """idg_intent_noise_f32: out[r, f] = the normal of (seed, stream_id, base_row + r, f) — the Z the intent kernels generate,
    at any width (the composed path of intent_mix draws it here)."""
    _require_device(out)
    n, d = out.shape
    check(lib.idg_intent_noise_f32(int(base_row), n, d, C.c_uint64(seed), C.c_uint64(stream_id), _row_base(out, base_row), _stream()),
          "idg_intent_noise_f32")
    return out


def intent_fwd_raw(X, W, T, F, row0=0, nrows=None, rows_bitmap=None, noise=None, seed=0, stream_id=0, noise_out=None, base_row=0):
    """idg_intent_fwd_f32 on global rows row0 .. row0 + nrows - 1: T = softmax(X . W) . W^T, F = X + T o Z.  The panels'
    first row is global row base_row (default 0: whole panels; row0 >= base_row); rows_bitmap is indexed by the global row.
    Leading dimensions are the tensors' row strides; noise / noise_out are contiguous [., d]."""
    _require_device(X, W, T, F, rows_bitmap, noise, noise_out)
    d, k = W.shape
    nrows = X.shape[0] - (int(row0) - int(base_row)) if nrows is None else nrows
    check(lib.idg_intent_fwd_f32(_row_base(X, base_row), _ld(X), int(row0), int(nrows), _ptr(W), d, k, _ptr(rows_bitmap),
                                 _row_base(noise, base_row), C.c_uint64(seed), C.c_uint64(stream_id), _row_base(T, base_row), _ld(T),
                                 _row_base(F, base_row), _ld(F), _row_base(noise_out, base_row), _stream()), "idg_intent_fwd_f32")
    return F, T


def intent_bwd_raw(gF, gT_in, rows_bitmap, X, W, gX, gW, row0=0, nrows=None, noise=None, seed=0, stream_id=0, base_row=0, ws=None,
                   gt_rows=None):
    """idg_intent_bwd_f32 on global rows row0 .. row0 + nrows - 1 (flagged rows only when rows_bitmap is given):
    gX = gF + gS . W^T, gW = X^T . gS + gT^T . P with gT = gT_in (at the rows of gt_rows, when given) + gF o Z; P and Z are
    recomputed."""
    _require_device(gF, gT_in, rows_bitmap, X, W, gX, gW, noise, gt_rows)
    d, k = W.shape
    nrows = X.shape[0] - (int(row0) - int(base_row)) if nrows is None else nrows
    if ws is None:
        ws = _cached_ws(_intent_ws, (d, k, X.device), lambda: max(int(lib.idg_intent_bwd_workspace_bytes(d, k)), 16), X.device)
    check(lib.idg_intent_bwd_f32(_row_base(gF, base_row), _ld(gF), _row_base(gT_in, base_row), 0 if gT_in is None else _ld(gT_in),
                                 _ptr(gt_rows), _ptr(rows_bitmap), _row_base(X, base_row), _ld(X), int(row0), int(nrows), _ptr(W), d, k,
                                 _row_base(noise, base_row), C.c_uint64(seed), C.c_uint64(stream_id), _row_base(gX, base_row), _ld(gX),
                                 _ptr(gW), _ptr(ws), _stream()), "idg_intent_bwd_f32")
    return gX, gW


class _IntentMix(torch.autograd.Function):
    """(F, T) of the intent layer at (d, k) = (64, 128) in one kernel per direction (csrc/idg_intent.hip).  Saved: X, W (and
    the noise panel when one was passed in); P is recomputed and Z regenerated from (seed, stream id, global row)."""

    @staticmethod
    def forward(ctx, X, W, row0, stream, noise):
        seed, sid = stream
        F, T = torch.empty_like(X), torch.empty_like(X)
        intent_fwd_raw(X, W, T, F, row0=row0, noise=noise, seed=seed, stream_id=sid, base_row=row0)
        ctx.save_for_backward(X, W, noise)
        ctx.args = (int(row0), seed, sid)
        return F, T

    @staticmethod
    def backward(ctx, gF, gT):
        X, W, noise = ctx.saved_tensors
        row0, seed, sid = ctx.args
        gF = torch.zeros_like(X) if gF is None else _f32c(gF, "gF")
        gT = None if gT is None else _f32c(gT, "gT")
        gX, gW = torch.empty_like(X), torch.empty_like(W)
        intent_bwd_raw(gF, gT, None, X, W, gX, gW, row0=row0, noise=noise, seed=seed, stream_id=sid, base_row=row0)
        return gX, gW, None, None, None


def intent_mix(X, W, row0=0, stream=None, noise=None):
    """BIGCF's intent layer (models/BIGCF.py:62-69) on the rows of X [n, d] with the intent matrix W [d, k]:
    T = softmax(X @ W, dim=1) @ W.T, F = X + T * Z; returns (F, T), differentiable in X and W.  Z ~ N(0, 1): `noise` [n, d]
    when given, else the counter-based normal of (seed, stream id, row0 + r, f) — row0 is the global row of X's first row,
    so the user and the item rows of one panel draw different noise from one stream.  (d, k) = (64, 128):
    idg_intent_fwd_f32 / idg_intent_bwd_f32; any other width composes torch operators with the same Z
    (idg_intent_noise_f32).  stream: (seed, stream id); default: the next one of the device seed's sequence."""
    for t, name in ((X, "X"), (W, "W"), (noise, "noise")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("intent_mix: %s must be float32 (got %s)" % (name, t.dtype))
    if X.dim() != 2 or W.dim() != 2:
        raise ValueError("intent_mix: X must be [n, d] and W [d, k], got %s and %s" % (tuple(X.shape), tuple(W.shape)))
    if X.shape[1] != W.shape[0]:
        raise ValueError("intent_mix: X %s and W %s do not fit (X [n, d], W [d, k])" % (tuple(X.shape), tuple(W.shape)))
    if X.shape[0] == 0:
        raise ValueError("intent_mix: X has 0 rows")
    if noise is not None and tuple(noise.shape) != tuple(X.shape):
        raise ValueError("intent_mix: noise %s must have X's shape %s" % (tuple(noise.shape), tuple(X.shape)))
    if int(row0) < 0:
        raise ValueError("intent_mix: row0 = %d is negative" % int(row0))
    if not (X.is_cuda and W.is_cuda and (noise is None or noise.is_cuda)):
        raise RuntimeError("intent_mix: runs on MI355X only (got X on %s, W on %s); there is no CPU fallback" % (X.device, W.device))
    stream = _next_noise_stream() if stream is None else stream
    noise = None if noise is None else _f32c(noise.detach(), "noise")
    if tuple(W.shape) == (64, 128):
        return _IntentMix.apply(_f32c(X, "X"), _f32c(W, "W"), int(row0), stream, noise)
    if noise is None:
        noise = intent_noise_raw(torch.empty(tuple(X.shape), dtype=torch.float32, device=X.device), stream[0], stream[1], base_row=row0)
    T = torch.softmax(X @ W, dim=1) @ W.t()
    return X + T * noise, T


# ----------------------------------------------------------------------------------- HCCF's hypergraph layer
_hyper_ws = {}


def _hyper_workspace(device, d=64, h=64):
    return _cached_ws(_hyper_ws, (d, h, device), lambda: max(int(lib.idg_hyper_latent_workspace_bytes(d, h)),
                                                             int(lib.idg_hyper_close_workspace_bytes(d, h)), 16), device)


def _mask_base(mask, base_row):
    """Pointer of GLOBAL row 0 of a contiguous uint8 / bool [., h] mask panel whose first row is global row base_row."""
    if mask is None:
        return None
    if mask.dtype not in (torch.uint8, torch.bool) or not mask.is_contiguous():
        raise TypeError("hyper mask must be a contiguous uint8 or bool panel (got %s, contiguous=%s)" % (mask.dtype, mask.is_contiguous()))
    return mask.data_ptr() - int(base_row) * int(mask.shape[1])


def _hyper_rows(P, row0, base_row, nrows):
    return P.shape[0] - (int(row0) - int(base_row)) if nrows is None else int(nrows)


def hyper_latent_raw(E0, W, X, L, row0=0, nrows=None, keep=1.0, mask=None, seed=0, stream_id=0, mask_out=None, base_row=0, ws=None):
    """idg_hyper_latent_f32 on global rows row0 .. row0 + nrows - 1: L [h, d] = H^T . X with H = M o (E0 . W) / keep.  The
    panels' (and masks') first row is global row base_row (default 0: whole panels; row0 >= base_row); leading dimensions are
    the tensors' row strides.  mask: uint8 / bool [., h], else the generator's of (seed, stream_id)."""
    _require_device(E0, W, X, L, mask, mask_out)
    d, h = W.shape
    ws = _hyper_workspace(E0.device, d, h) if ws is None else ws
    check(lib.idg_hyper_latent_f32(_row_base(E0, base_row), _ld(E0), _ptr(W), d, h, _row_base(X, base_row), _ld(X), int(row0),
                                   _hyper_rows(X, row0, base_row, nrows), float(keep), _mask_base(mask, base_row), C.c_uint64(seed),
                                   C.c_uint64(stream_id), _ptr(L), _mask_base(mask_out, base_row), _ptr(ws), _stream()),
          "idg_hyper_latent_f32")
    return L


def hyper_expand_raw(E0, W, L, Y, row0=0, nrows=None, keep=1.0, mask=None, seed=0, stream_id=0, side=None, next=None, total=None,
                     base_row=0):
    """idg_hyper_expand_f32: Y = H . L; with side and next: next = side + Y; with total: total += next (+= Y without side)."""
    _require_device(E0, W, L, Y, mask, side, next, total)
    d, h = W.shape
    ld = lambda t: 0 if t is None else _ld(t)  # noqa: E731
    check(lib.idg_hyper_expand_f32(_row_base(E0, base_row), _ld(E0), _ptr(W), d, h, _ptr(L), int(row0), _hyper_rows(Y, row0, base_row, nrows),
                                   float(keep), _mask_base(mask, base_row), C.c_uint64(seed), C.c_uint64(stream_id),
                                   _row_base(Y, base_row), _ld(Y), _row_base(side, base_row), ld(side), _row_base(next, base_row), ld(next),
                                   _row_base(total, base_row), ld(total), _stream()), "idg_hyper_expand_f32")
    return Y


def hyper_bwd_raw(E0, W, X, gY, L, gL, gX, gHb, row0=0, nrows=None, keep=1.0, mask=None, seed=0, stream_id=0, accumulate=False,
                  base_row=0):
    """idg_hyper_bwd_f32: gX += H . gL;  gHb = (accumulate ? gHb : 0) + M o (gY . L^T + X . gL^T) / keep."""
    _require_device(E0, W, X, gY, L, gL, gX, gHb, mask)
    d, h = W.shape
    check(lib.idg_hyper_bwd_f32(_row_base(E0, base_row), _ld(E0), _ptr(W), d, h, _row_base(X, base_row), _ld(X), _row_base(gY, base_row),
                                _ld(gY), _ptr(L), _ptr(gL), int(row0), _hyper_rows(X, row0, base_row, nrows), float(keep),
                                _mask_base(mask, base_row), C.c_uint64(seed), C.c_uint64(stream_id), _row_base(gX, base_row), _ld(gX),
                                _row_base(gHb, base_row), _ld(gHb), int(bool(accumulate)), _stream()), "idg_hyper_bwd_f32")
    return gX, gHb


def hyper_close_raw(E0, W, gHb, gE0, gW, row0=0, nrows=None, base_row=0, ws=None):
    """idg_hyper_close_f32: gE0 += gHb . W^T;  gW [d, h] = E0^T . gHb (stored)."""
    _require_device(E0, W, gHb, gE0, gW)
    d, h = W.shape
    ws = _hyper_workspace(E0.device, d, h) if ws is None else ws
    check(lib.idg_hyper_close_f32(_row_base(E0, base_row), _ld(E0), _ptr(W), d, h, _row_base(gHb, base_row), _ld(gHb), int(row0),
                                  _hyper_rows(E0, row0, base_row, nrows), _row_base(gE0, base_row), _ld(gE0), _ptr(gW), _ptr(ws), _stream()),
          "idg_hyper_close_f32")
    return gE0, gW


class _HyperMix(torch.autograd.Function):
    """Y = H . (H^T . X) at (d, h) = (64, 64) on csrc/idg_hyper.hip's four kernels.  Saved: E0, W, X, L (64 x 64) and the mask
    panel when one was passed in; H is recomputed and the mask regenerated from (seed, stream id, global row)."""

    @staticmethod
    def forward(ctx, E0, W, X, row0, keep, stream, mask):
        seed, sid = stream
        L, Y = torch.empty_like(W), torch.empty_like(X)
        kw = dict(row0=row0, keep=keep, mask=mask, seed=seed, stream_id=sid, base_row=row0)
        hyper_latent_raw(E0, W, X, L, **kw)
        hyper_expand_raw(E0, W, L, Y, **kw)
        ctx.save_for_backward(E0, W, X, L, mask)
        ctx.kw = kw
        return Y

    @staticmethod
    def backward(ctx, gY):
        E0, W, X, L, mask = ctx.saved_tensors
        kw = ctx.kw
        gY = _f32c(gY, "gY")
        gL, gW = torch.empty_like(L), torch.empty_like(W)
        gX, gE0 = torch.zeros_like(X), torch.zeros_like(E0)
        gHb = torch.empty((E0.shape[0], W.shape[1]), dtype=torch.float32, device=E0.device)
        hyper_latent_raw(E0, W, gY, gL, **kw)
        hyper_bwd_raw(E0, W, X, gY, L, gL, gX, gHb, accumulate=False, **kw)
        hyper_close_raw(E0, W, gHb, gE0, gW, row0=kw["row0"], base_row=kw["base_row"])
        return gE0, gW, gX, None, None, None, None


def hyper_mix(E0, W, X, row0=0, keep=1.0, stream=None, mask=None):
    """One side of HCCF's hypergraph layer (models/HCCF.py:56-74): with Hb = E0 @ W [n, h] and H = M * Hb / keep it returns
    Y = H @ (H.T @ X) [n, d], differentiable in E0, W and X.  M ~ Bernoulli(keep): `mask` (uint8 / bool [n, h]) when given, else
    the counter-based keep function of (seed, stream id, row0 + r, c) — row0 is the global row of the panels' first row, so
    the two sides of one panel draw different masks from one stream; keep >= 1 keeps everything.  (d, h) = (64, 64): the four
    kernels of csrc/idg_hyper.hip, H never stored; any other width composes torch operators under autograd, and draws a
    missing mask with torch.rand (NOT the kernels' function of the stream).  stream: (seed, stream id); default: the next one
    of the device seed's sequence."""
    for t, name in ((E0, "E0"), (W, "W"), (X, "X")):
        if t.dtype != torch.float32:
            raise TypeError("hyper_mix: %s must be float32 (got %s)" % (name, t.dtype))
    if E0.dim() != 2 or W.dim() != 2 or X.dim() != 2 or E0.shape[1] != W.shape[0] or X.shape[0] != E0.shape[0]:
        raise ValueError("hyper_mix: E0 [n, d], W [d, h] and X [n, d'] do not fit (got %s, %s, %s)"
                         % (tuple(E0.shape), tuple(W.shape), tuple(X.shape)))
    if E0.shape[0] == 0:
        raise ValueError("hyper_mix: E0 has 0 rows")
    if mask is not None and tuple(mask.shape) != (E0.shape[0], W.shape[1]):
        raise ValueError("hyper_mix: mask %s must be [n, h] = %s" % (tuple(mask.shape), (E0.shape[0], W.shape[1])))
    if int(row0) < 0 or not float(keep) > 0.0:
        raise ValueError("hyper_mix: row0 = %d must not be negative and keep = %g must be positive" % (int(row0), float(keep)))
    if not (E0.is_cuda and W.is_cuda and X.is_cuda and (mask is None or mask.is_cuda)):
        raise RuntimeError("hyper_mix: runs on MI355X only (got E0 on %s, W on %s, X on %s); there is no CPU fallback"
                           % (E0.device, W.device, X.device))
    keep = float(keep)
    if tuple(W.shape) == (64, 64) and X.shape[1] == 64:
        stream = _next_noise_stream() if stream is None else stream
        mask = None if mask is None else mask.contiguous()
        return _HyperMix.apply(_f32c(E0, "E0"), _f32c(W, "W"), _f32c(X, "X"), int(row0), keep, stream, mask)
    Hb = E0 @ W
    if mask is None and keep < 1.0:
        mask = torch.rand(Hb.shape, device=Hb.device) < keep
    H = Hb if mask is None else Hb * (mask.to(Hb.dtype) / min(keep, 1.0))
    return H @ (H.t() @ X)


# ----------------------------------------------------------------------------------- InfoNCE


def infonce_pair_raw(view1, view2, users, items, num_users, temperature, g1=None, g2=None, loss=None, dedup=True,
                     grad_scale=1.0, accumulate=False, ws=None, planned=False):
    """idg_infonce_pair_f32: loss[2] = InfoNCE over unique(users) rows and over num_users + unique(items) rows of
    the two [n, d] view panels; g1 / g2 (optional, pre-zeroed) receive d(loss[0] + loss[1]) / d view rows."""
    _require_device(view1, view2, users, items, g1, g2, loss)
    view1, view2 = _f32c(view1, "view1"), _f32c(view2, "view2")
    users, items = _i64c(users, "users"), _i64c(items, "items")
    n, d = view1.shape
    B = users.shape[0]
    if view2.shape != view1.shape or items.shape[0] != B:
        raise ValueError("infonce_pair_raw: view panels / id lists of different shapes")
    if ws is None:
        if planned:
            raise ValueError("infonce_pair_raw: planned=True needs the workspace idg_infonce_plan wrote into")
        ws = _cached_ws(_ssl_ws, (n, B, d, view1.device), lambda: lib.idg_infonce_workspace_bytes(n, B, d), view1.device)
    if loss is None:
        loss = torch.empty(2, dtype=torch.float32, device=view1.device)
    check(lib.idg_infonce_pair_f32(_ptr(view1), _ptr(view2), n, d, _ptr(users), _ptr(items), B, int(num_users),
                                   int(bool(dedup)) | (native.IDG_SSL_PLANNED if planned else 0), float(temperature), _ptr(loss),
                                   _ptr(g1), _ptr(g2), float(grad_scale),
                                   int(bool(accumulate)), _ptr(ws), _stream()),
          "idg_infonce_pair_f32")
    return loss


class _InfoNCEPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, view1, view2, users, items, num_users, temperature, dedup):
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g1 = torch.zeros_like(view1, memory_format=torch.contiguous_format) if need1 else None
        g2 = torch.zeros_like(view2, memory_format=torch.contiguous_format) if need2 else None
        loss = infonce_pair_raw(view1.detach(), view2.detach(), users, items, num_users, temperature, g1, g2, dedup=dedup)
        ctx.saved = (g1, g2)
        return loss.sum()

    @staticmethod
    def backward(ctx, grad_out):
        g1, g2 = ctx.saved
        return (None if g1 is None else g1.mul_(grad_out), None if g2 is None else g2.mul_(grad_out), None, None, None, None,
                None)


def infonce_pair(view1, view2, users, items, num_users, temperature, dedup=True):
    """get_InfoNCE_loss(view1[U-rows of unique(users)], view2[...]) + get_InfoNCE_loss(... unique(items) rows ...)
    — the self-supervised term of SimGCL / XSimGCL (models/SimGCL.py:79-84) — as one differentiable operator on
    the two [n, d] view panels (users first).  dedup=False: the id lists as they are, duplicates included (SGL)."""
    return _InfoNCEPair.apply(view1, view2, users, items, num_users, temperature, bool(dedup))


def spmm_rows_width(d):
    """True when idg_spmm_epi_f32 can produce a row subset (out_rows) at width d: the tiled widths; any other width
    forms every row (x_rows has no such limit)."""
    return int(d) in (32, 64, 128, 256, 512)


def users_bitmap(users, n, out=None):
    """int32 bitmap of n bits with the bits of `users` set (idg_bpr_touch_rows with every slot of the triple a user)."""
    if out is None:
        out = torch.empty((n + 31) // 32, dtype=torch.int32, device=users.device)
    bpr_touch_rows_raw(users, users, users, 0, out, clear_bits=n)
    return out


class _EncodeRows(torch.autograd.Function):
    """rows users of R_hat . Wt (R_hat [U, I] rectangular, Wt [I, 2d]): the product at those rows only (out_rows); the
    backward is the transposed handle's product over the rows of the incoming gradient (x_rows) — [I, 2d]."""

    @staticmethod
    def forward(ctx, Wt, graph, users):
        Wt = _f32c(Wt.detach(), "Wt")
        users = _i64c(users, "users")
        bits = users_bitmap(users, graph.n_rows)
        panel = torch.empty((graph.n_rows, Wt.shape[1]), dtype=torch.float32, device=Wt.device)
        spmm_epi_raw(graph, Wt, Y=panel, out_rows=bits if spmm_rows_width(Wt.shape[1]) else None)
        out = torch.empty((users.shape[0], Wt.shape[1]), dtype=torch.float32, device=Wt.device)
        rows_gather_raw(out, panel, users)
        ctx.graph = graph
        ctx.save_for_backward(users, bits)
        return out

    @staticmethod
    def backward(ctx, g):
        users, bits = ctx.saved_tensors
        graph = ctx.graph
        # the batch's gradient rows into a panel read at the bitmap's rows only (a repeated user's rows are summed)
        gp = torch.zeros((graph.n_rows, g.shape[1]), dtype=torch.float32, device=g.device)
        gp.index_put_((users,), _f32c(g, "g"), accumulate=True)
        out = torch.empty((graph.n_cols, g.shape[1]), dtype=torch.float32, device=g.device)
        spmm_epi_raw(graph.T, gp, Y=out, x_rows=bits)
        return out, None, None


def encode_rows(graph, Wt, users):
    """(R_hat . Wt)[users] — the encoder layer of CVGA (models/CVGA.py:40-43, without its bias) at the batch's rows only."""
    return _EncodeRows.apply(Wt, graph, users)
