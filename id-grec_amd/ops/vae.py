"""csrc/idg_vae.hip: CVGA's multinomial likelihood and VAE head."""
import ctypes as C

import torch

from .. import native
from ..native import check, lib
from ._base import _cached_ws, _f32c, _i64c, _ptr, _require_device, _require_ids, _stream
from .graph import _next_noise_stream


def multinomial_nll_workspace(B, I, d, device):
    """A private idg_multinomial_nll_f32 buffer: O(chunks B d + B), never B x I.  It also keeps the row statistics of the
    last forward call made with it."""
    return torch.empty(int(lib.idg_multinomial_nll_workspace_bytes(int(B), int(I), int(d))), dtype=torch.uint8, device=device)


def multinomial_nll_raw(Z, W, c, users, indptr, items, values, loss=None, upstream=None, gZ=None, gW=None, gc=None,
                        stats_ready=False, ws=None):
    """idg_multinomial_nll_f32: loss[1] = (1/B) sum_b (n_b LSE_b - sum_i x_bi l_bi), l = Z W^T + c, x_b = row users[b] of
    the device train CSR (indptr, items, values) — get_ELBO_loss's BCE term on decode(z) (models/CVGA.py:55-75).
    gZ / gW / gc (all or none, stored): its gradients scaled by `upstream` (device [1]; None = 1).  stats_ready: the row
    statistics in `ws` from a forward call on the same inputs are reused.  Returns (loss, ws)."""
    _require_device(Z, W, c, users, indptr, items, values, loss, upstream, gZ, gW, gc, ws)
    _require_ids(users)
    B, d = Z.shape
    I = W.shape[0]
    for t, name in ((Z, "Z"), (W, "W"), (c, "c"), (values, "values")):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("multinomial_nll_raw: %s must be contiguous float32" % name)
    if W.shape[1] != d or c.shape[0] != I or indptr.dtype != torch.int64 or items.dtype != torch.int32:
        raise TypeError("multinomial_nll_raw: Z [B, d], W [I, d], c [I], indptr int64, items int32")
    if ws is None:
        ws = multinomial_nll_workspace(B, I, d, Z.device)
    if loss is None and gZ is None:
        loss = torch.empty(1, dtype=torch.float32, device=Z.device)
    check(lib.idg_multinomial_nll_f32(_ptr(Z), _ptr(W), _ptr(c), B, I, d, _ptr(users), _ptr(indptr), _ptr(items), _ptr(values),
                                      _ptr(loss), _ptr(upstream), _ptr(gZ), _ptr(gW), _ptr(gc),
                                      native.IDG_NLL_STATS_READY if stats_ready else 0, _ptr(ws), _stream()),
          "idg_multinomial_nll_f32")
    return loss, ws


class _MultinomialNLL(torch.autograd.Function):
    """The forward keeps its workspace (the row max / sum-exp statistics); the backward runs only the gradient pass."""

    @staticmethod
    def forward(ctx, Z, W, c, users, indptr, items, values):
        Z, W, c = _f32c(Z.detach(), "Z"), _f32c(W.detach(), "W"), _f32c(c.detach(), "c")
        users = _i64c(users, "users")
        loss, ws = multinomial_nll_raw(Z, W, c, users, indptr, items, values)
        ctx.save_for_backward(Z, W, c, users, indptr, items, values)
        ctx.ws = ws
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        Z, W, c, users, indptr, items, values = ctx.saved_tensors
        up = g.to(torch.float32).reshape(1).contiguous()
        gZ, gW, gc = torch.empty_like(Z), torch.empty_like(W), torch.empty_like(c)
        multinomial_nll_raw(Z, W, c, users, indptr, items, values, upstream=up, gZ=gZ, gW=gW, gc=gc, stats_ready=True,
                            ws=ctx.ws)
        return gZ, gW, gc, None, None, None, None


def multinomial_nll(Z, W, c, users, indptr, items, values):
    """-mean_b sum_i log_softmax(Z W^T + c)_bi x_bi (losses.py:54) with x the users' rows of the device train CSR, as a
    0-d tensor differentiable w.r.t. Z [B, d], W [I, d] and c [I]; the [B, I] logits are never stored."""
    return _MultinomialNLL.apply(Z, W, c, users, indptr, items, values)


_head_ws = {}


def _head_workspace(B, device):
    return _cached_ws(_head_ws, (int(B), device), lambda: lib.idg_vae_head_workspace_bytes(int(B)), device)


def _head_args(name, pre, users, bias, pre_rows, **rows_d):
    """Shapes of the head's operands: pre [*, 2d] (row b read at pre_rows[b], else b), bias [2d], users / pre_rows
    contiguous int64 [B]; every tensor in rows_d contiguous float32 with B rows of the stated width.  Returns (B, d)."""
    _require_ids(users)
    B = int(users.shape[0])
    if pre.dtype != torch.float32 or not pre.is_contiguous() or pre.dim() != 2 or pre.shape[1] % 2:
        raise TypeError("%s: pre must be a contiguous float32 [*, 2d] tensor" % name)
    d = int(pre.shape[1]) // 2
    if bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != 2 * d:
        raise TypeError("%s: bias must be a contiguous float32 [2d] tensor" % name)
    if pre_rows is None:
        if pre.shape[0] < B:
            raise ValueError("%s: pre has fewer than B rows" % name)
    else:
        _require_ids(pre_rows)
        if pre_rows.shape[0] != B:
            raise ValueError("%s: pre_rows must hold B ids" % name)
    for key, (t, width) in rows_d.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, width * d)):
            raise TypeError("%s: %s must be a contiguous float32 [%d, %d] tensor" % (name, key, B, width * d))
    return B, d


def vae_head_raw(pre, users, bias, p, seed, stream_id, z=None, kl=None, eps=None, pre_rows=None, eps_out=None, keep_out=None,
                 with_kl=True):
    """idg_vae_head_fwd_f32: z [B, d] = eps * exp(logvar / 2) + mu with (mu | logvar) = dropout_p(pre[row] + bias) and
    kl [1] = -0.5 / B^2 sum (1 + logvar - mu^2 - exp logvar) (models/CVGA.py:40-67, losses.py:55).  pre: [B, 2d], or a
    [*, 2d] panel read at pre_rows[b].  eps: [B, d] injected noise; None: drawn from (seed, stream_id, user, feature).
    with_kl=False: z only (kl is NULL for the library and None here).  Returns (z, kl)."""
    _require_device(pre, users, bias, z, kl, eps, pre_rows, eps_out, keep_out)
    B, d = _head_args("vae_head_raw", pre, users, bias, pre_rows, z=(z, 1), eps=(eps, 1), eps_out=(eps_out, 1),
                      keep_out=(keep_out, 2))
    if kl is not None and (kl.dtype != torch.float32 or kl.numel() < 1):
        raise TypeError("vae_head_raw: kl must be a float32 tensor of at least one element")
    if z is None:
        z = torch.empty((B, d), dtype=torch.float32, device=pre.device)
    if not with_kl:
        kl = None
    elif kl is None:
        kl = torch.empty(1, dtype=torch.float32, device=pre.device)
    check(lib.idg_vae_head_fwd_f32(_ptr(pre), 2 * d, _ptr(pre_rows), _ptr(users), B, d, _ptr(bias), float(p), C.c_uint64(seed),
                                   C.c_uint64(stream_id), _ptr(eps), _ptr(z), _ptr(kl), _ptr(eps_out), _ptr(keep_out),
                                   _ptr(_head_workspace(B, pre.device)), _stream()), "idg_vae_head_fwd_f32")
    return z, kl


def vae_head_bwd_raw(pre, users, bias, p, seed, stream_id, gz, gpre, upstream_kl=None, gbias=None, eps=None, pre_rows=None,
                     gpre_rows=None):
    """idg_vae_head_bwd_f32: gpre rows (gpre_rows[b], distinct, or b) <- keep * d/d(mu | logvar) of the decoder loss (through
    gz = d L / d z) plus upstream_kl * KL; gbias (optional) <- their column sums in batch order.  keep and eps are
    regenerated from the forward's (seed, stream_id) — or eps is the same injected tensor."""
    _require_device(pre, users, bias, gz, gpre, upstream_kl, gbias, eps, pre_rows, gpre_rows)
    B, d = _head_args("vae_head_bwd_raw", pre, users, bias, pre_rows, gz=(gz, 1), eps=(eps, 1))
    if gpre.dtype != torch.float32 or not gpre.is_contiguous() or gpre.dim() != 2 or gpre.shape[1] != 2 * d:
        raise TypeError("vae_head_bwd_raw: gpre must be a contiguous float32 [*, 2d] tensor")
    if gpre_rows is None:
        if gpre.shape[0] < B:
            raise ValueError("vae_head_bwd_raw: gpre has fewer than B rows")
    else:
        _require_ids(gpre_rows)
        if gpre_rows.shape[0] != B:
            raise ValueError("vae_head_bwd_raw: gpre_rows must hold B ids")
    if gbias is not None and (gbias.dtype != torch.float32 or not gbias.is_contiguous() or gbias.numel() != 2 * d):
        raise TypeError("vae_head_bwd_raw: gbias must be a contiguous float32 [2d] tensor")
    if upstream_kl is not None and (upstream_kl.dtype != torch.float32 or upstream_kl.numel() < 1):
        raise TypeError("vae_head_bwd_raw: upstream_kl must be a float32 tensor of at least one element")
    check(lib.idg_vae_head_bwd_f32(_ptr(pre), 2 * d, _ptr(pre_rows), _ptr(users), B, d, _ptr(bias), float(p), C.c_uint64(seed),
                                   C.c_uint64(stream_id), _ptr(eps), _ptr(gz), _ptr(upstream_kl), _ptr(gpre), 2 * d,
                                   _ptr(gpre_rows), _ptr(gbias), _stream()), "idg_vae_head_bwd_f32")


class _VaeHead(torch.autograd.Function):
    """(z, kl) of the batch rows pre [B, 2d]; the backward regenerates the mask and eps from (seed, stream_id)."""

    @staticmethod
    def forward(ctx, pre, bias, users, p, seed, stream_id, eps):
        pre, bias = _f32c(pre.detach(), "pre"), _f32c(bias.detach(), "bias")
        users = _i64c(users, "users")
        z, kl = vae_head_raw(pre, users, bias, p, seed, stream_id, eps=eps)
        ctx.save_for_backward(pre, bias, users, eps)
        ctx.meta = (float(p), int(seed), int(stream_id))
        return z, kl[0]

    @staticmethod
    def backward(ctx, gz, gkl):
        pre, bias, users, eps = ctx.saved_tensors
        p, seed, sid = ctx.meta
        gz = None if gz is None else _f32c(gz, "gz")
        up = (torch.zeros(1, dtype=torch.float32, device=pre.device) if gkl is None
              else gkl.to(torch.float32).reshape(1).contiguous())
        gpre, gbias = torch.empty_like(pre), torch.empty_like(bias)
        vae_head_bwd_raw(pre, users, bias, p, seed, sid, gz, gpre, upstream_kl=up, gbias=gbias, eps=eps)
        return gpre, gbias, None, None, None, None, None


def vae_head(pre, bias, users, p, stream=None, eps=None):
    """CVGA's head on the batch's encoder rows pre [B, 2d] (models/CVGA.py:40-67): dropout p on (pre + bias), split into
    mu / logvar, z = mu + eps * exp(logvar / 2), and the KL term.  Returns (z [B, d], kl 0-d), differentiable w.r.t. pre
    and bias.  stream: (seed, stream id) of the mask and the noise (default: the next noise stream)."""
    seed, sid = _next_noise_stream() if stream is None else stream
    if eps is not None:
        eps = _f32c(eps.detach(), "eps")
    return _VaeHead.apply(pre, bias, users, p, seed, sid, eps)
