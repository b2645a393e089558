"""csrc/idg_sccf.hip: SCCF's second-order in-batch contrast."""
import torch

from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ptr, _require_device, _require_ids, _stream


_sccf_ws_cache = {}


def _sccf_ws_bytes(B, d):
    size = int(lib.idg_sccf_workspace_bytes(int(B), int(d)))
    if size == 0:
        raise ValueError("sccf_workspace: B = %d, d = %d is not built (1 <= d <= 256, 1 <= B < 2^22)" % (B, d))
    return size


def sccf_workspace(B, d, device):
    """A private idg_sccf_loss_f32 scratch buffer (the padded operands, the per-tile partial gradient rows, the plan)."""
    return torch.empty(_sccf_ws_bytes(B, d), dtype=torch.uint8, device=device)


def sccf_loss_raw(final, users, pos, num_users, temperature, g_final=None, g_ego=None, loss=None, upstream=None,
                  accumulate=True, plan_ws=None, ws=None):
    """idg_sccf_loss_f32: loss[2] = [-up, down] of SCCF (models/SCCF.py:54-81) over the batch's rows users / num_users + pos
    of `final`.  g_final (optional): d(up[0] loss[0] + up[1] loss[1]) / d final with `upstream` = up (device [2]; None =
    ones); accumulate=True adds into the rows the batch touches, False STORES them (the rows of
    bpr_touch_rows_raw(users, pos, pos)) and, given g_ego (a second panel, never g_final), stores zeros to its same rows.
    plan_ws: a BPR workspace holding bpr_plan_raw(users, pos, pos, ...) of this batch; None: in-call."""
    _require_device(final, users, pos, g_final, g_ego, loss, upstream)
    _require_ids(users, pos)
    n, d = final.shape
    B = users.shape[0]
    if pos.shape[0] != B:
        raise ValueError("sccf_loss_raw: id lists of different lengths")
    if ws is None:
        ws = _cached_ws(_sccf_ws_cache, (int(B), int(d), final.device), lambda: _sccf_ws_bytes(B, d), final.device)
    if loss is None:
        loss = torch.empty(2, dtype=torch.float32, device=final.device)
    check(lib.idg_sccf_loss_f32(_ptr(final), n, d, _ptr(users), _ptr(pos), B, int(num_users), float(temperature), _ptr(loss),
                                _ptr(upstream), _ptr(g_final), _ptr(g_ego), int(bool(accumulate)), _ptr(plan_ws), _ptr(ws),
                                _stream()),
          "idg_sccf_loss_f32")
    return loss


class _SCCFLoss(torch.autograd.Function):
    """The forward computes the two losses only; the backward runs the call again with the incoming pair as upstream."""

    @staticmethod
    def forward(ctx, final, users, pos, num_users, temperature):
        _require_device(final, users, pos)
        fin = _f32c(final.detach(), "final")
        users, pos = _i64c(users, "users"), _i64c(pos, "pos")
        loss = sccf_loss_raw(fin, users, pos, num_users, temperature)
        ctx.save_for_backward(fin, users, pos)
        ctx.meta = (int(num_users), float(temperature))
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_up, g_down):
        fin, users, pos = ctx.saved_tensors
        num_users, temperature = ctx.meta
        up = torch.stack([g.to(torch.float32).reshape(()) for g in (g_up, g_down)]).contiguous()
        g_final = torch.zeros_like(fin)
        sccf_loss_raw(fin, users, pos, num_users, temperature, g_final, upstream=up, accumulate=True)
        return g_final, None, None, None, None


def sccf_loss(final, user, positive, num_users, temperature):
    """SCCF's loss pair (neg_up, down) as 0-d tensors, differentiable w.r.t. the [num_users + num_items, d] panel:
    neg_up = -mean_i log f(a_i.b_i), down = log(mean over distinct users x distinct positives of f(a_k.b_l) cu_k ci_l),
    f(s) = exp(s / T) + exp(s^2 / T), a / b the normalised rows (models/SCCF.py:54-81)."""
    return _SCCFLoss.apply(final, user, positive, num_users, temperature)
