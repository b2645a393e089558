"""csrc/idg_nance.hip: LightCCF / LightCSCF's neighbour-aggregation loss and the row regulariser."""
import torch

from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ptr, _require_device, _require_ids, _stream


_na_ws_cache = {}


def _na_ws_bytes(B, d):
    size = int(lib.idg_na_nce_workspace_bytes(int(B), int(d)))
    if size == 0:
        raise ValueError("na_nce_workspace: B = %d, d = %d is not built (1 <= d <= 256, 1 <= B < 2^22)" % (B, d))
    return size


def na_nce_workspace(B, d, device):
    """A private idg_na_nce_f32 / idg_reg_rows_f32 scratch buffer (the padded operands, the per-tile partials, the plan)."""
    return torch.empty(_na_ws_bytes(B, d), dtype=torch.uint8, device=device)


def _na_ws(B, d, device):
    return _cached_ws(_na_ws_cache, (int(B), int(d), device), lambda: _na_ws_bytes(B, d), device)


def na_nce_loss_raw(final, users, pos, num_users, temperature, margin=None, grad_scale=1.0, g_final=None, loss=None,
                    upstream=None, accumulate=True, plan_ws=None, ws=None):
    """idg_na_nce_f32: loss[1] = grad_scale * mean_i -log(f(a_i.b_i) / sum_j f(a_i.(a_j + b_j)) + 1e-5) over the batch's
    rows users / num_users + pos of `final` (models/LightCCF.py:81-94; with margin = lambda_margin, models/LightCSCF.py:93-104;
    margin None: LightCCF's f).  g_final (optional): upstream * d loss / d final (upstream: device [1]; None = 1);
    accumulate=True adds into the rows the batch touches, False STORES every row of the plan.  plan_ws: a BPR workspace
    holding bpr_plan_raw(users, pos, neg or pos, ...) of this batch; None: in-call."""
    _require_device(final, users, pos, g_final, loss, upstream)
    _require_ids(users, pos)
    n, d = final.shape
    B = users.shape[0]
    if pos.shape[0] != B:
        raise ValueError("na_nce_loss_raw: id lists of different lengths")
    if margin is not None and not 0.0 <= float(margin) <= 2.0:
        raise ValueError("na_nce_loss_raw: margin must be in [0, 2] (None: LightCCF's form), got %r" % (margin,))
    if ws is None:
        ws = _na_ws(B, d, final.device)
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=final.device)
    check(lib.idg_na_nce_f32(_ptr(final), n, d, _ptr(users), _ptr(pos), B, int(num_users), float(temperature),
                             -1.0 if margin is None else float(margin), float(grad_scale), _ptr(loss), _ptr(upstream),
                             _ptr(g_final), int(bool(accumulate)), _ptr(plan_ws), _ptr(ws), _stream()),
          "idg_na_nce_f32")
    return loss


def reg_rows_raw(ego, users, pos, neg, num_users, reg_lambda, g_ego=None, g_final=None, loss=None, plan_ws=None, ws=None):
    """idg_reg_rows_f32: loss[1] = reg_lambda * 1/2 (sum |e_u|^2 + sum |e_p|^2 + sum |e_n|^2) / B over the ego rows of the
    batch (duplicates counted); its gradient rows STORED to g_ego and zeros STORED to the same rows of g_final (both
    optional).  plan_ws: a BPR workspace holding bpr_plan_raw(users, pos, neg, ...) of this batch; None: in-call."""
    _require_device(ego, users, pos, neg, g_ego, g_final, loss)
    _require_ids(users, pos, neg)
    n, d = ego.shape
    B = users.shape[0]
    if pos.shape[0] != B or neg.shape[0] != B:
        raise ValueError("reg_rows_raw: id lists of different lengths")
    if ws is None:
        ws = _na_ws(B, d, ego.device)
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=ego.device)
    check(lib.idg_reg_rows_f32(_ptr(ego), n, d, _ptr(users), _ptr(pos), _ptr(neg), B, int(num_users), float(reg_lambda),
                               _ptr(loss), _ptr(g_ego), _ptr(g_final), _ptr(plan_ws), _ptr(ws), _stream()),
          "idg_reg_rows_f32")
    return loss


class _RegRows(torch.autograd.Function):
    """The forward computes the loss only; the backward stores the gradient rows into a zeroed panel and scales them."""

    @staticmethod
    def forward(ctx, ego, users, pos, neg, num_users, reg_lambda):
        _require_device(ego, users, pos, neg)
        e = _f32c(ego.detach(), "ego")
        users, pos, neg = _i64c(users, "users"), _i64c(pos, "pos"), _i64c(neg, "neg")
        loss = reg_rows_raw(e, users, pos, neg, num_users, reg_lambda)
        ctx.save_for_backward(e, users, pos, neg)
        ctx.meta = (int(num_users), float(reg_lambda))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        e, users, pos, neg = ctx.saved_tensors
        num_users, reg_lambda = ctx.meta
        g_ego = torch.zeros_like(e)
        reg_rows_raw(e, users, pos, neg, num_users, reg_lambda, g_ego=g_ego)
        return g_ego.mul_(g.to(torch.float32)), None, None, None, None, None


def reg_rows_loss(ego, user, positive, negative, num_users, reg_lambda):
    """reg_lambda * get_reg_loss(ego[user], ego[num_users + positive], ego[num_users + negative]) as a 0-d tensor,
    differentiable w.r.t. the ego panel (LightCSCF on LightGCN: the regulariser without a BPR term)."""
    return _RegRows.apply(ego, user, positive, negative, num_users, reg_lambda)


class _NaNceLoss(torch.autograd.Function):
    """The forward computes the loss only; the backward runs the call again with the incoming scalar as upstream."""

    @staticmethod
    def forward(ctx, final, users, pos, num_users, temperature, margin, weight):
        _require_device(final, users, pos)
        fin = _f32c(final.detach(), "final")
        users, pos = _i64c(users, "users"), _i64c(pos, "pos")
        loss = na_nce_loss_raw(fin, users, pos, num_users, temperature, margin, weight)
        ctx.save_for_backward(fin, users, pos)
        ctx.meta = (int(num_users), float(temperature), margin, float(weight))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        fin, users, pos = ctx.saved_tensors
        num_users, temperature, margin, weight = ctx.meta
        up = g.to(torch.float32).reshape(1).contiguous()
        g_final = torch.zeros_like(fin)
        na_nce_loss_raw(fin, users, pos, num_users, temperature, margin, weight, g_final, upstream=up, accumulate=True)
        return g_final, None, None, None, None, None, None


def na_nce_loss(final, user, positive, num_users, temperature, margin=None, weight=1.0):
    """weight * the neighbour-aggregation loss of LightCCF (margin None) / LightCSCF (margin = lambda_margin) as a 0-d tensor,
    differentiable w.r.t. the [num_users + num_items, d] panel."""
    return _NaNceLoss.apply(final, user, positive, num_users, temperature, margin, weight)
