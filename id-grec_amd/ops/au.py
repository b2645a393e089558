"""csrc/idg_au.hip: DirectAU's alignment and uniformity loss."""
import torch

from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ptr, _require_device, _require_ids, _stream


_au_ws_cache = {}


def align_uniform_workspace(B, d, device):
    """A private idg_align_uniform_f32 scratch buffer (O(B d): the pair matrix is never stored)."""
    return torch.empty(int(lib.idg_align_uniform_workspace_bytes(int(B), int(d))), dtype=torch.uint8, device=device)


def align_uniform_raw(final_panel, ego_panel, users, pos, num_users, gamma, reg_lambda, g_final=None, g_ego=None,
                      loss=None, upstream=None, accumulate=True, plan_ws=None, ws=None):
    """idg_align_uniform_f32: loss[3] = [align, gamma * uniform, reg_lambda * reg] of DirectAU (models/DirectAU.py:59-79)
    over the batch's rows users / num_users + pos of final_panel (reg over the same rows of ego_panel).
    g_final / g_ego (optional): d(align + gamma * uniform) / d final and d(reg) / d ego — the same tensor for the MF
    encoder (final_panel is ego_panel) — each scaled by `upstream` (device [3], d total / d loss[k]; None = ones).
    accumulate=True adds into the rows the batch touches; False STORES them (the rows of
    bpr_touch_rows_raw(users, pos, pos)), nothing else is written.  plan_ws: a BPR workspace holding
    bpr_plan_raw(users, pos, pos, ...) of this batch (index-only, prepared ahead on a side stream); None: in-call."""
    _require_device(final_panel, ego_panel, users, pos, g_final, g_ego, loss, upstream)
    _require_ids(users, pos)
    n, d = final_panel.shape
    B = users.shape[0]
    if pos.shape[0] != B or ego_panel.shape != final_panel.shape:
        raise ValueError("align_uniform_raw: id lists / panels of different shapes")
    if ws is None:
        ws = _cached_ws(_au_ws_cache, (int(B), int(d), final_panel.device),
                        lambda: lib.idg_align_uniform_workspace_bytes(int(B), int(d)), final_panel.device)
    if loss is None:
        loss = torch.empty(3, dtype=torch.float32, device=final_panel.device)
    check(lib.idg_align_uniform_f32(_ptr(final_panel), _ptr(ego_panel), n, d, _ptr(users), _ptr(pos), B, int(num_users),
                                    float(gamma), float(reg_lambda), _ptr(loss), _ptr(upstream), _ptr(g_final), _ptr(g_ego),
                                    int(bool(accumulate)), _ptr(plan_ws), _ptr(ws), _stream()),
          "idg_align_uniform_f32")
    return loss


class _AlignUniform(torch.autograd.Function):
    """The forward computes the losses only; the backward runs the call again with the three incoming gradient
    scalars (the pair pass twice — this is the path of widths the fused step does not cover)."""

    @staticmethod
    def forward(ctx, final_panel, ego_panel, users, pos, num_users, gamma, reg_lambda):
        _require_device(final_panel, ego_panel, users, pos)
        fin = _f32c(final_panel.detach(), "final_panel")
        same = ego_panel is final_panel
        ego = fin if same else _f32c(ego_panel.detach(), "ego_panel")
        users, pos = _i64c(users, "users"), _i64c(pos, "pos")
        loss = align_uniform_raw(fin, ego, users, pos, num_users, gamma, reg_lambda)
        ctx.save_for_backward(fin, ego, users, pos)
        ctx.meta = (int(num_users), float(gamma), float(reg_lambda), same)
        return loss[0], loss[1], loss[2]

    @staticmethod
    def backward(ctx, g_align, g_unif, g_reg):
        fin, ego, users, pos = ctx.saved_tensors
        num_users, gamma, reg_lambda, same = ctx.meta
        up = torch.stack([g.to(torch.float32).reshape(()) for g in (g_align, g_unif, g_reg)]).contiguous()
        g_final = torch.zeros_like(fin)
        g_ego = g_final if same else torch.zeros_like(ego)
        align_uniform_raw(fin, fin if same else ego, users, pos, num_users, gamma, reg_lambda, g_final, g_ego,
                          upstream=up, accumulate=True)
        return g_final, (None if same else g_ego), None, None, None, None, None


class _AlignUniformSame(torch.autograd.Function):
    """final == ego (the MF encoder): one differentiable input that receives both gradients."""

    @staticmethod
    def forward(ctx, panel, users, pos, num_users, gamma, reg_lambda):
        return _AlignUniform.forward(ctx, panel, panel, users, pos, num_users, gamma, reg_lambda)

    @staticmethod
    def backward(ctx, g_align, g_unif, g_reg):
        return (_AlignUniform.backward(ctx, g_align, g_unif, g_reg)[0], None, None, None, None, None)


def align_uniform_loss(final_panel, ego_panel, users, pos, num_users, gamma, reg_lambda):
    """DirectAU's loss triple (align, gamma * uniform, reg_lambda * reg) as 0-d tensors, differentiable w.r.t. both
    [num_users + num_items, d] panels: get_align_loss(a, b), gamma * (get_uniform_loss(a) + get_uniform_loss(b)) / 2 and
    reg_lambda * get_reg_loss(ego rows) with a = final[users], b = final[num_users + pos] (models/DirectAU.py:59-79).
    Passing the same tensor twice is the MF encoder."""
    if ego_panel is final_panel:
        return _AlignUniformSame.apply(final_panel, users, pos, num_users, gamma, reg_lambda)
    return _AlignUniform.apply(final_panel, ego_panel, users, pos, num_users, gamma, reg_lambda)
