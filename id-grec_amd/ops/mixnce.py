"""csrc/idg_mixnce.hip: MixRec's in-batch mixing terms."""
import torch

from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ptr, _require_device, _require_ids, _stream


MIX_NCE_MAX_WIDTH = 256
_mix_ws_cache = {}


def _mix_ws_bytes(B, d):
    nbytes = int(lib.idg_mix_nce_workspace_bytes(int(B), int(d)))
    if nbytes == 0:
        raise ValueError("mix_nce_workspace: sizes that are not built (B=%d, d=%d; d <= %d)" % (B, d, MIX_NCE_MAX_WIDTH))
    return nbytes


def mix_nce_workspace(B, d, device):
    """A private idg_mix_nce_f32 buffer (the normalised copies, per-row statistics and ordered partial sums: O(chunks B d))."""
    return torch.empty(_mix_ws_bytes(B, d), dtype=torch.uint8, device=device)


def mix_nce_raw(panel, num_users, users, pos, neg, user_perm, item_perm, nu, user_beta, item_beta, temperature, ssl_weight,
                loss=None, upstream=None, g_panel=None, ws=None):
    """idg_mix_nce_f32 (include/idgrec.h states the math): loss[0] = (1 - item_beta) x the rectangular term of the users' rows
    against the mixed negatives, loss[1] = ssl_weight x (the users' side + the positives' side), on rows of `panel` [n, d]
    (users first).  user_perm / item_perm: int64 [B] permutations, nu: float32 [B], all on the device.  g_panel (None: losses
    only): the gradient of upstream[0] loss[0] + upstream[1] loss[1] (device [2]; None = ones) w.r.t. the panel is ADDED
    into the batch's rows.  Returns the loss pair."""
    _require_device(panel, users, pos, neg, user_perm, item_perm, nu, loss, upstream, g_panel, ws)
    _require_ids(users, pos, neg, user_perm, item_perm)
    if panel.dim() != 2 or panel.dtype != torch.float32 or not panel.is_contiguous():
        raise TypeError("mix_nce_raw: panel must be a contiguous float32 [n, d] tensor")
    n, d = panel.shape
    B = int(users.shape[0])
    if B < 1 or any(tuple(t.shape) != (B,) for t in (users, pos, neg, user_perm, item_perm, nu)):
        raise ValueError("mix_nce_raw: users, pos, neg, both permutations and nu are [B] with B >= 1")
    if nu.dtype != torch.float32 or not nu.is_contiguous():
        raise TypeError("mix_nce_raw: nu must be contiguous float32")
    if g_panel is not None and (g_panel.dtype != torch.float32 or not g_panel.is_contiguous() or g_panel.shape != panel.shape):
        raise ValueError("mix_nce_raw: g_panel must be a contiguous float32 tensor of the panel's shape")
    if not 0 < int(num_users) < n:
        raise ValueError("mix_nce_raw: num_users = %d of %d panel rows" % (int(num_users), n))
    if ws is None:
        ws = _cached_ws(_mix_ws_cache, (B, int(d), panel.device), lambda: _mix_ws_bytes(B, d), panel.device)
    if loss is None:
        loss = torch.empty(2, dtype=torch.float32, device=panel.device)
    check(lib.idg_mix_nce_f32(_ptr(panel), n, d, int(num_users), _ptr(users), _ptr(pos), _ptr(neg), B, _ptr(user_perm),
                              _ptr(item_perm), _ptr(nu), float(user_beta), float(item_beta), float(temperature), float(ssl_weight),
                              _ptr(loss), _ptr(upstream), _ptr(g_panel), _ptr(ws), _stream()), "idg_mix_nce_f32")
    return loss


class _MixNCE(torch.autograd.Function):
    """The forward computes the two losses only; the backward runs the call again with the incoming gradient scalars."""

    @staticmethod
    def forward(ctx, panel, meta):
        det = _f32c(panel.detach(), "panel")
        loss = mix_nce_raw(det, *meta)
        ctx.save_for_backward(det)
        ctx.meta = meta
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g0, g1):
        (det,) = ctx.saved_tensors
        up = torch.stack([g0.to(torch.float32).reshape(()), g1.to(torch.float32).reshape(())]).contiguous()
        g = torch.zeros_like(det)
        mix_nce_raw(det, *ctx.meta, upstream=up, g_panel=g)
        return g, None


def mix_nce(panel, num_users, users, pos, neg, user_perm, item_perm, nu, user_beta, item_beta, temperature, ssl_weight):
    """MixRec's two contrastive loss entries as 0-d tensors, differentiable w.r.t. the panel (see mix_nce_raw)."""
    _require_device(panel, users, pos, neg, user_perm, item_perm, nu)
    meta = (int(num_users), _i64c(users, "users"), _i64c(pos, "pos"), _i64c(neg, "neg"), _i64c(user_perm, "user_perm"),
            _i64c(item_perm, "item_perm"), _f32c(nu, "nu"), float(user_beta), float(item_beta), float(temperature),
            float(ssl_weight))
    return _MixNCE.apply(panel, meta)
