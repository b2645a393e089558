"""csrc/idg_svdnce.hip: LightGCL's low-rank products and SVD-view contrastive terms."""
import torch

from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ld, _ptr, _require_device, _require_ids, _stream


LOWRANK_MAX_RANK = 16
SVD_NCE_MAX_WIDTH = 256
_lowrank_ws_cache = {}
_svd_nce_ws_cache = {}


def _rows_panel(who, t, name):
    """A float32 [rows, w] device tensor read where it lies: unit column stride, any row stride >= w."""
    if t.dim() != 2 or t.dtype != torch.float32:
        raise TypeError("%s: %s must be a float32 [rows, width] tensor" % (who, name))
    if t.shape[1] > 1 and t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _lowrank_sizes(who, A, d, n):
    q = int(A.shape[1])
    if not 1 <= q <= LOWRANK_MAX_RANK:
        raise ValueError("%s: rank %d (1 .. %d are built)" % (who, q, LOWRANK_MAX_RANK))
    if not 1 <= d <= SVD_NCE_MAX_WIDTH:
        raise ValueError("%s: width %d (1 .. %d are built)" % (who, d, SVD_NCE_MAX_WIDTH))
    if n < 1:
        raise ValueError("%s: no rows" % who)
    return q


def _lowrank_rows(who, A, a_rows, n_default):
    if a_rows is None:
        return int(n_default)
    _require_ids(a_rows)
    if a_rows.dim() != 1:
        raise ValueError("%s: a_rows must be a 1-d id list" % who)
    return int(a_rows.shape[0])


def lowrank_project_raw(A, X, out=None, a_rows=None, accumulate=False, ws=None):
    """idg_lowrank_project_f32: out [q, d] (+)= sum_r A[a_rows[r] if a_rows is given else r]^T X[r], a tall deterministic
    reduction.  A [*, q] and X [n, d] are read with their own row strides; a_rows: int64 [n] rows of A (may repeat)."""
    _require_device(A, X, out, a_rows, ws)
    A, X = _rows_panel("lowrank_project_raw", A, "A"), _rows_panel("lowrank_project_raw", X, "X")
    n, d = int(X.shape[0]), int(X.shape[1])
    q = _lowrank_sizes("lowrank_project_raw", A, d, n)
    if _lowrank_rows("lowrank_project_raw", A, a_rows, A.shape[0]) != n:
        raise ValueError("lowrank_project_raw: %d rows of A for %d rows of X" % (A.shape[0] if a_rows is None else a_rows.shape[0], n))
    if out is None:
        if accumulate:
            raise ValueError("lowrank_project_raw: accumulate needs `out`")
        out = torch.empty((q, d), dtype=torch.float32, device=X.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (q, d):
        raise ValueError("lowrank_project_raw: out must be a contiguous float32 [%d, %d] tensor" % (q, d))
    if ws is None:
        ws = _cached_ws(_lowrank_ws_cache, (n, q, d, X.device), lambda: lib.idg_lowrank_project_workspace_bytes(n, q, d), X.device)
    check(lib.idg_lowrank_project_f32(_ptr(A), _ld(A), _ptr(a_rows), _ptr(X), _ld(X), n, q, d, _ptr(out), int(bool(accumulate)),
                                      _ptr(ws), _stream()), "idg_lowrank_project_f32")
    return out


def lowrank_expand_raw(A, P, Y=None, a_rows=None, scale=1.0, accumulate=False):
    """idg_lowrank_expand_f32: Y[r] (+)= scale A[a_rows[r] if a_rows is given else r] P for every row r of Y.  A [*, q],
    P [q, d]; Y [n, d] is written with its own row stride."""
    _require_device(A, P, Y, a_rows)
    A = _rows_panel("lowrank_expand_raw", A, "A")
    P = _f32c(P, "P")
    if P.dim() != 2 or P.shape[0] != A.shape[1]:
        raise ValueError("lowrank_expand_raw: P is %s, A is [*, %d]" % (tuple(P.shape), A.shape[1]))
    d = int(P.shape[1])
    n = _lowrank_rows("lowrank_expand_raw", A, a_rows, A.shape[0])
    q = _lowrank_sizes("lowrank_expand_raw", A, d, n)
    if Y is None:
        if accumulate:
            raise ValueError("lowrank_expand_raw: accumulate needs `Y`")
        Y = torch.empty((n, d), dtype=torch.float32, device=P.device)
    elif (Y.dim() != 2 or Y.dtype != torch.float32 or tuple(Y.shape) != (n, d) or (d > 1 and Y.stride(1) != 1)
          or (n > 1 and Y.stride(0) < d)):
        raise ValueError("lowrank_expand_raw: Y must be a float32 [%d, %d] tensor with unit column stride" % (n, d))
    check(lib.idg_lowrank_expand_f32(_ptr(A), _ld(A), _ptr(a_rows), _ptr(P), n, q, d, float(scale), int(bool(accumulate)),
                                     _ptr(Y), _ld(Y), _stream()), "idg_lowrank_expand_f32")
    return Y


class _LowrankProject(torch.autograd.Function):
    """out = A[rows]^T X, differentiable w.r.t. X (the factors are constants): gX = A[rows] g_out."""

    @staticmethod
    def forward(ctx, X, A, a_rows):
        ctx.A, ctx.a_rows = A, a_rows
        return lowrank_project_raw(A, X.detach(), a_rows=a_rows)

    @staticmethod
    def backward(ctx, g):
        return lowrank_expand_raw(ctx.A, _f32c(g, "grad"), a_rows=ctx.a_rows), None, None


class _LowrankExpand(torch.autograd.Function):
    """Y = scale A[rows] P, differentiable w.r.t. P: gP = scale A[rows]^T gY."""

    @staticmethod
    def forward(ctx, P, A, a_rows, scale):
        ctx.A, ctx.a_rows, ctx.scale = A, a_rows, scale
        return lowrank_expand_raw(A, P.detach(), a_rows=a_rows, scale=scale)

    @staticmethod
    def backward(ctx, g):
        gP = lowrank_project_raw(ctx.A, g, a_rows=ctx.a_rows)
        return (gP if ctx.scale == 1.0 else gP * ctx.scale), None, None, None


def lowrank_project(A, X, a_rows=None):
    """A[a_rows]^T X as a [q, d] tensor, differentiable w.r.t. X (see lowrank_project_raw)."""
    _require_device(A, X, a_rows)
    return _LowrankProject.apply(X, A.detach(), None if a_rows is None else _i64c(a_rows, "a_rows"))


def lowrank_expand(A, P, a_rows=None, scale=1.0):
    """scale A[a_rows] P as an [n, d] tensor, differentiable w.r.t. P (see lowrank_expand_raw)."""
    _require_device(A, P, a_rows)
    return _LowrankExpand.apply(P, A.detach(), None if a_rows is None else _i64c(a_rows, "a_rows"), float(scale))


def _svd_nce_args(final_panel, ego_panel, row0, N, AS, P, ids, temperature):
    """The checks of the SVD-view contrastive calls that need no device; returns (B, d, q)."""
    if not float(temperature) > 0:
        raise ValueError("svd_nce: temperature must be positive (got %r)" % (temperature,))
    if final_panel.dim() != 2 or ego_panel.shape != final_panel.shape:
        raise ValueError("svd_nce: the final and ego panels must both be [n, d]")
    n, d = final_panel.shape
    row0, N = int(row0), int(N)
    if N < 1 or row0 < 0 or row0 + N > n:
        raise ValueError("svd_nce: rows [%d, %d) are not inside the [%d, %d] panel" % (row0, row0 + N, n, d))
    if d > SVD_NCE_MAX_WIDTH:
        raise ValueError("svd_nce: width %d (up to %d is built)" % (d, SVD_NCE_MAX_WIDTH))
    if AS.dim() != 2 or AS.shape[0] != N or not 1 <= AS.shape[1] <= LOWRANK_MAX_RANK:
        raise ValueError("svd_nce: the factor rows are %s, the side has %d rows (rank 1 .. %d)" % (tuple(AS.shape), N, LOWRANK_MAX_RANK))
    q = int(AS.shape[1])
    if tuple(P.shape) != (q, d):
        raise ValueError("svd_nce: P is %s, expected [%d, %d]" % (tuple(P.shape), q, d))
    if ids.dim() != 1 or ids.shape[0] < 1:
        raise ValueError("svd_nce: empty batch")
    return int(ids.shape[0]), int(d), q


def _svd_nce_ws_bytes(B, N, d, q):
    nbytes = int(lib.idg_svd_nce_workspace_bytes(int(B), int(N), int(d), int(q)))
    if nbytes == 0:
        raise ValueError("svd_nce_workspace: sizes that are not built (B=%d, N=%d, d=%d, q=%d)" % (B, N, d, q))
    return nbytes


def svd_nce_workspace(B, N, d, q, device):
    """A private idg_svd_nce_f32 buffer: the padded copies, per-chunk statistics and ordered partial sums
    (O((N + chunks B) d)), never B x N."""
    return torch.empty(_svd_nce_ws_bytes(B, N, d, q), dtype=torch.uint8, device=device)


def svd_nce_raw(final_panel, ego_panel, row0, N, AS, P, ids, temperature, loss=None, upstream=None, g_final=None, g_ego=None,
                dP=None, ws=None):
    """idg_svd_nce_f32 (include/idgrec.h states the math), one side: with g_b = ego_panel[row0 + ids[b]] + AS[ids[b]] P and
    s_bj = <g_b, final_panel[row0 + j]> / temperature, loss[0] = mean_b log(sum_{j < N} exp(s_bj) + 1e-8) and
    loss[1] = mean_b clamp(<final_panel[row0 + ids[b]], g_b> / temperature, -5, 5).  g_final, g_ego [n, d] and dP [q, d] (all
    or none): the gradient of upstream[0] loss[0] + upstream[1] loss[1] (device [2]; None = ones) is ADDED into the two panels
    — the caller zeroes — and dP is stored.  Returns the loss pair."""
    B, d, q = _svd_nce_args(final_panel, ego_panel, row0, N, AS, P, ids, temperature)
    outs = (g_final, g_ego, dP)
    grads = any(t is not None for t in outs)
    if grads and any(t is None for t in outs):
        raise ValueError("svd_nce_raw: g_final, g_ego and dP go together")
    _require_device(final_panel, ego_panel, AS, P, ids, loss, upstream, g_final, g_ego, dP, ws)
    _require_ids(ids)
    for t, shape in ((final_panel, None), (ego_panel, None), (AS, None), (P, None), (g_final, final_panel.shape),
                     (g_ego, final_panel.shape), (dP, (q, d))):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("svd_nce_raw: panels, factors and P must be contiguous float32")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("svd_nce_raw: a gradient output of shape %s, expected %s" % (tuple(t.shape), tuple(shape)))
    dev = final_panel.device
    if ws is None:
        ws = _cached_ws(_svd_nce_ws_cache, (B, int(N), d, q, dev), lambda: _svd_nce_ws_bytes(B, N, d, q), dev)
    if loss is None:
        loss = torch.empty(2, dtype=torch.float32, device=dev)
    check(lib.idg_svd_nce_f32(_ptr(final_panel), _ptr(ego_panel), int(row0), int(N), d, _ptr(AS), q, _ptr(P), _ptr(ids), B,
                              float(temperature), _ptr(loss), _ptr(upstream), _ptr(g_final), _ptr(g_ego), _ptr(dP), _ptr(ws),
                              _stream()), "idg_svd_nce_f32")
    return loss


class _SvdNCE(torch.autograd.Function):
    """The forward computes the two losses only; the backward runs the call again with the incoming gradient scalars."""

    @staticmethod
    def forward(ctx, final_panel, ego_panel, P, meta):
        det = [_f32c(t.detach(), "panel") for t in (final_panel, ego_panel, P)]
        row0, N, AS, ids, temperature = meta
        loss = svd_nce_raw(det[0], det[1], row0, N, AS, det[2], ids, temperature)
        ctx.save_for_backward(*det)
        ctx.meta = meta
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g0, g1):
        F, E, P = ctx.saved_tensors
        row0, N, AS, ids, temperature = ctx.meta
        up = torch.stack([g0.to(torch.float32).reshape(()), g1.to(torch.float32).reshape(())]).contiguous()
        gF, gE, dP = torch.zeros_like(F), torch.zeros_like(E), torch.empty_like(P)
        svd_nce_raw(F, E, row0, N, AS, P, ids, temperature, upstream=up, g_final=gF, g_ego=gE, dP=dP)
        return gF, gE, dP, None


def svd_nce_loss(final_panel, ego_panel, row0, N, AS, P, ids, temperature):
    """LightGCL's two contrastive terms of one side — (log-sum-exp term, clamped positive term) — as 0-d tensors,
    differentiable w.r.t. the final panel, the ego panel and P (see svd_nce_raw); AS, the side's factor rows times the
    singular values, is a constant."""
    _svd_nce_args(final_panel, ego_panel, row0, N, AS, P, ids, temperature)
    _require_device(final_panel, ego_panel, AS, P, ids)
    meta = (int(row0), int(N), _f32c(AS.detach(), "AS"), _i64c(ids, "ids"), float(temperature))
    return _SvdNCE.apply(final_panel, ego_panel, P, meta)
