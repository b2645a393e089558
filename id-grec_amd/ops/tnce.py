"""csrc/idg_tnce.hip: CGCL's full-table contrastive terms."""
import ctypes as C

import torch

from .. import native
from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ptr, _require_device, _require_ids, _stream


TABLE_NCE_MAX_WIDTH = 256


def _table_nce_args(table_panel, row0, N, query_panels, query_ids, pos_ids, weights, temperature):
    """The checks of the full-table contrastive calls that need no device; returns (nq, B, d)."""
    nq = len(query_panels)
    if not 1 <= nq <= native.IDG_TNCE_MAX_QUERY_BLOCKS:
        raise ValueError("table_nce: %d query blocks (1 .. %d share one table)" % (nq, native.IDG_TNCE_MAX_QUERY_BLOCKS))
    if len(query_ids) != nq or len(weights) != nq:
        raise ValueError("table_nce: %d query panels, %d id lists, %d weights" % (nq, len(query_ids), len(weights)))
    if not float(temperature) > 0:
        raise ValueError("table_nce: temperature must be positive (got %r)" % (temperature,))
    if table_panel.dim() != 2:
        raise ValueError("table_nce: the table panel must be [n, d]")
    n, d = table_panel.shape
    row0, N = int(row0), int(N)
    if N < 1 or row0 < 0 or row0 + N > n:
        raise ValueError("table_nce: rows [%d, %d) are not inside the [%d, %d] panel" % (row0, row0 + N, n, d))
    if d > TABLE_NCE_MAX_WIDTH:
        raise ValueError("table_nce: width %d (up to %d is built)" % (d, TABLE_NCE_MAX_WIDTH))
    B = int(pos_ids.shape[0])
    if B < 1:
        raise ValueError("table_nce: empty batch")
    for k in range(nq):
        if query_panels[k].dim() != 2 or query_panels[k].shape[1] != d:
            raise ValueError("table_nce: query panel %d is %s, the table is [*, %d]" % (k, tuple(query_panels[k].shape), d))
        if query_ids[k].dim() != 1 or query_ids[k].shape[0] != B:
            raise ValueError("table_nce: id list %d has %s entries, pos_ids %d" % (k, tuple(query_ids[k].shape), B))
    return nq, B, int(d)


def _tnce_ws_bytes(B, N, d, nq):
    nbytes = int(lib.idg_table_nce_workspace_bytes(int(B), int(N), int(d), int(nq)))
    if nbytes == 0:
        raise ValueError("table_nce_workspace: sizes that are not built (B=%d, N=%d, d=%d, nq=%d)" % (B, N, d, nq))
    return nbytes


def table_nce_workspace(B, N, d, nq, device):
    """A private idg_table_nce_f32 buffer: the normalised copies, per-row statistics and ordered partial sums
    (O((N + chunks nq B) d)), never B x N."""
    return torch.empty(_tnce_ws_bytes(B, N, d, nq), dtype=torch.uint8, device=device)


_tnce_ws_cache = {}


def table_nce_raw(table_panel, row0, N, query_panels, query_ids, pos_ids, weights, temperature, loss=None, upstream=None,
                  g_table=None, g_queries=None, ws=None):
    """idg_table_nce_f32: loss[k] = -weights[k] sum_b log(exp(s_b,pos / tau) / sum_{j < N} exp(s_bj / tau) + 1e-7) with
    s = normalize(query_panels[k][query_ids[k]]) . normalize(table_panel[row0 : row0 + N])^T and the positive of query b at
    table row pos_ids[b] (models/CGCL.py:95-215's six terms; losses.get_InfoNCE_loss_all's expression).  g_table [n, d] and
    g_queries (one panel per block; both or neither): the gradients of sum_k upstream[k] loss[k] (device [nq]; None = ones)
    are ADDED into them — the caller zeroes, and may pass one tensor in several roles.  Returns the loss vector [nq]."""
    nq, B, d = _table_nce_args(table_panel, row0, N, query_panels, query_ids, pos_ids, weights, temperature)
    grads = g_table is not None or g_queries is not None
    if grads and (g_table is None or g_queries is None or len(g_queries) != nq):
        raise ValueError("table_nce_raw: g_table and one gradient panel per query block go together")
    gq = list(g_queries) if grads else []
    _require_device(table_panel, pos_ids, loss, upstream, g_table, ws, *query_panels, *query_ids, *gq)
    _require_ids(pos_ids, *query_ids)
    for t, ref in [(table_panel, None), (g_table, table_panel)] + [(q, None) for q in query_panels] + list(zip(gq, query_panels)):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("table_nce_raw: panels must be contiguous float32")
        if ref is not None and t.shape != ref.shape:
            raise ValueError("table_nce_raw: a gradient panel of shape %s for a panel of shape %s" % (tuple(t.shape), tuple(ref.shape)))
    dev = table_panel.device
    if ws is None:
        ws = _cached_ws(_tnce_ws_cache, (B, int(N), d, nq, dev), lambda: _tnce_ws_bytes(B, N, d, nq), dev)
    if loss is None:
        loss = torch.empty(nq, dtype=torch.float32, device=dev)
    vp = C.c_void_p * nq
    check(lib.idg_table_nce_f32(_ptr(table_panel), int(row0), int(N), d, nq, vp(*[_ptr(q) for q in query_panels]),
                                vp(*[_ptr(i) for i in query_ids]), B, _ptr(pos_ids), (C.c_float * nq)(*[float(w) for w in weights]),
                                float(temperature), _ptr(loss), _ptr(upstream), _ptr(g_table),
                                vp(*[_ptr(g) for g in gq]) if grads else None, _ptr(ws), _stream()), "idg_table_nce_f32")
    return loss


class _TableNCE(torch.autograd.Function):
    """The forward computes the losses only; the backward runs the call again with the incoming gradient scalars.  Distinct
    tensors among (table, query panels) are the differentiable inputs; a tensor in several roles receives the sum."""

    @staticmethod
    def forward(ctx, meta, *panels):
        roles, row0, N, ids, pos_ids, weights, temperature = meta
        det = [_f32c(p.detach(), "panel") for p in panels]
        table, queries = det[roles[0]], [det[r] for r in roles[1:]]
        loss = table_nce_raw(table, row0, N, queries, ids, pos_ids, weights, temperature)
        ctx.save_for_backward(*det)
        ctx.meta = meta
        return tuple(loss[k] for k in range(len(queries)))

    @staticmethod
    def backward(ctx, *gl):
        det = ctx.saved_tensors
        roles, row0, N, ids, pos_ids, weights, temperature = ctx.meta
        up = torch.stack([g.to(torch.float32).reshape(()) for g in gl]).contiguous()
        grads = [torch.zeros_like(p) for p in det]
        table_nce_raw(det[roles[0]], row0, N, [det[r] for r in roles[1:]], ids, pos_ids, weights, temperature, upstream=up,
                      g_table=grads[roles[0]], g_queries=[grads[r] for r in roles[1:]])
        return (None,) + tuple(grads)


def table_nce_loss(table_panel, row0, N, query_panels, query_ids, pos_ids, weights, temperature):
    """The full-table contrastive terms as nq 0-d tensors, differentiable w.r.t. the table panel and every query panel (see
    table_nce_raw).  The same tensor may be the table panel and a query panel, or serve several blocks: it is one
    differentiable input and its gradients add."""
    _table_nce_args(table_panel, row0, N, query_panels, query_ids, pos_ids, weights, temperature)
    _require_device(table_panel, pos_ids, *query_panels, *query_ids)
    panels, roles = [], []
    for t in [table_panel] + list(query_panels):
        for i, p in enumerate(panels):
            if p is t:
                roles.append(i)
                break
        else:
            roles.append(len(panels))
            panels.append(t)
    ids = [_i64c(i, "query_ids") for i in query_ids]
    meta = (tuple(roles), int(row0), int(N), ids, _i64c(pos_ids, "pos_ids"), [float(w) for w in weights], float(temperature))
    return _TableNCE.apply(meta, *panels)
