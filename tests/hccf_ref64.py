"""HCCF's hypergraph layer, its closed-form gradients and the whole training step stated once more, in plain torch and (by
default) float64: what tests/test_gpu_hccf.py holds the kernels of csrc/idg_hyper.hip, ops.hyper_mix, the fused chain
(idgrec_amd/hccf.py) and the plugin against, and what tests/test_hccf_host.py pins to the reference's own numbers
(tests/golden/hccf_small*.npz) without a GPU.  Nothing of the library is imported here.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick for how far a correct float32 evaluation may sit from the reference (band()).

Masks: one per layer and side, a bool / uint8 [n_s, h] tensor or None (everything kept); `masks` of the step functions is
None or a [K, n, h] tensor / a list of K [n, h] tensors, users first."""
import numpy as np
import torch

from tests.egcf_ref64 import adam64, band, dense_operator, deterministic, errors, infonce64  # noqa: F401

__all__ = ["adam64", "band", "dense_operator", "deterministic", "errors", "infonce64"]


def unpack_masks(packed):
    """The fixture's bit-packed masks uint8 [.., n, 8] -> bool tensor [.., n, 64]."""
    return torch.from_numpy(np.unpackbits(np.asarray(packed), axis=-1).astype(bool))


def hyper64(E0, W, mask, keep, dtype=torch.float64):
    """H = M o (E0 . W) / keep (F.dropout's scaling by 1 / (1 - p) with p = 1 - keep)."""
    Hb = E0.to(dtype) @ W.to(dtype)
    scale = 1.0 if keep >= 1.0 else 1.0 / keep
    if mask is None:
        return Hb * scale if scale != 1.0 else Hb
    return Hb * (mask.to(Hb.device, dtype) * scale)


def layer64(E0, W, X, mask, keep, dtype=torch.float64):
    """(Y, L, H) of one side: L = H^T . X [h, d], Y = H . L (models/HCCF.py: HGNN)."""
    H = hyper64(E0, W, mask, keep, dtype)
    L = H.t() @ X.to(dtype)
    return H @ L, L, H


def layer_grads64(E0, W, X, gY, mask, keep, dtype=torch.float64):
    """The layer's closed-form gradients for an upstream gY: (gL, H . gL [what the layer adds to gX], M o gH / keep [what it
    adds to gHb]) with gL = H^T . gY and gH = gY . L^T + X . gL^T."""
    _, L, H = layer64(E0, W, X, mask, keep, dtype)
    X, gY = X.to(dtype), gY.to(dtype)
    gL = H.t() @ gY
    gH = gY @ L.t() + X @ gL.t()
    scale = 1.0 if keep >= 1.0 else 1.0 / keep
    gHb = gH * scale if mask is None else gH * (mask.to(gH.device, dtype) * scale)
    return gL, H @ gL, gHb


def close64(E0, W, gHb, dtype=torch.float64):
    """(gHb . W^T [what the layers add to gE0], gW = E0^T . gHb)."""
    E0, W, gHb = E0.to(dtype), W.to(dtype), gHb.to(dtype)
    return gHb @ W.t(), E0.t() @ gHb


def _side_masks(masks, l, U):
    if masks is None:
        return None, None
    m = masks[l]
    return m[:U], m[U:]


def aggregate64(A, E0, Wu, Wi, U, K, masks, keep, dtype=torch.float64):
    """models/HCCF.py: aggregate() on a dense operator: (final = the SUM of the K + 1 layers, [S_l], [Y_l], [X_l])."""
    A = A.to(dtype)
    X = [E0.to(dtype)]
    S, Y = [], []
    for l in range(K):
        mu, mi = _side_masks(masks, l, U)
        S.append(A @ X[-1])
        yu = layer64(X[0][:U], Wu, X[-1][:U], mu, keep, dtype)[0]
        yi = layer64(X[0][U:], Wi, X[-1][U:], mi, keep, dtype)[0]
        Y.append(torch.cat([yu, yi]))
        X.append(S[-1] + Y[-1])
    final = X[0]
    for x in X[1:]:
        final = final + x
    return final, S, Y, X


def losses64(final, S, Y, E0, Wu, Wi, users, pos, neg, U, reg_lambda, ssl_lambda, t, dtype=torch.float64):
    """HCCF.forward's three losses [bpr, reg_lambda * reg, ssl_lambda * ssl] from the aggregated panels."""
    ue, pe, ne = final[users], final[U + pos], final[U + neg]
    x = (ue * pe).sum(dim=1) - (ue * ne).sum(dim=1)
    bpr = torch.mean(-torch.log(torch.sigmoid(x) + 10e-8))
    reg = sum(1 / 2 * blk.norm(2).pow(2) / float(blk.shape[0]) for blk in (E0[users], E0[U + pos], E0[U + neg], Wu, Wi))
    ssl = 0.
    for s, y in zip(S, Y):
        s = s.detach()
        ssl = ssl + infonce64(s[users], y[users], t, dtype) + infonce64(s[U + pos], y[U + pos], t, dtype)
    return torch.stack([bpr, reg_lambda * reg, ssl_lambda * ssl])


def step64(A, E0, Wu, Wi, users, pos, neg, K, masks, keep, reg_lambda, ssl_lambda, t, U, dtype=torch.float64):
    """HCCF.forward and its backward by autograd: (losses [3], (dE0, dWu, dWi), final, [S_l], [Y_l]) in `dtype`."""
    E0, Wu, Wi = (p.detach().to(dtype).clone().requires_grad_(True) for p in (E0, Wu, Wi))
    users, pos, neg = users.long(), pos.long(), neg.long()
    with deterministic():
        final, S, Y, _ = aggregate64(A, E0, Wu, Wi, U, K, masks, keep, dtype)
        losses = losses64(final, S, Y, E0, Wu, Wi, users, pos, neg, U, reg_lambda, ssl_lambda, t, dtype)
        grads = torch.autograd.grad(losses.sum(), (E0, Wu, Wi))
    return losses.detach(), grads, final.detach(), [s.detach() for s in S], [y.detach() for y in Y]


def step_closed64(A, E0, Wu, Wi, users, pos, neg, K, masks, keep, reg_lambda, ssl_lambda, t, U, dtype=torch.float64):
    """The same step with the backward the fused chain runs: autograd only through the three losses (as functions of final,
    the Y_l and the parameters' own rows), the layers by layer_grads64 / close64 in the order
        gX_K = gFinal;  l = K-1 .. 0:  gS_l = gX_l+1,  gY_l = gX_l+1 + d ssl / d Y_l,  gL_l = H_l^T gY_l,
        gHb += M_l o (gY_l L_l^T + X_l gL_l^T) / keep,  gX_l = gFinal + A gS_l + H_l gL_l   (A symmetric)
        gW_s = E0_s^T gHb,  gE0_s = gX_0 + gHb W_s^T + the regulariser's rows.
    Returns (losses, (dE0, dWu, dWi))."""
    A = A.to(dtype)
    E0, Wu, Wi = (p.detach().to(dtype) for p in (E0, Wu, Wi))
    users, pos, neg = users.long(), pos.long(), neg.long()
    with deterministic():
        final, S, Y, X = aggregate64(A, E0, Wu, Wi, U, K, masks, keep, dtype)
        leaves = [final.clone().requires_grad_(True)] + [y.clone().requires_grad_(True) for y in Y]
        e0, wu, wi = (p.clone().requires_grad_(True) for p in (E0, Wu, Wi))
        losses = losses64(leaves[0], S, leaves[1:], e0, wu, wi, users, pos, neg, U, reg_lambda, ssl_lambda, t, dtype)
        g = torch.autograd.grad(losses.sum(), leaves + [e0, wu, wi], allow_unused=True)
    gFinal, gYssl, (rE0, rWu, rWi) = g[0], g[1:K + 1], g[K + 1:]
    gX = gFinal
    gHb = [torch.zeros((U, Wu.shape[1]), dtype=dtype, device=E0.device), torch.zeros((E0.shape[0] - U, Wi.shape[1]), dtype=dtype, device=E0.device)]
    for l in range(K - 1, -1, -1):
        gS, gY = gX, gX + gYssl[l]
        mu, mi = _side_masks(masks, l, U)
        _, au, hu = layer_grads64(E0[:U], Wu, X[l][:U], gY[:U], mu, keep, dtype)
        _, ai, hi = layer_grads64(E0[U:], Wi, X[l][U:], gY[U:], mi, keep, dtype)
        gHb[0], gHb[1] = gHb[0] + hu, gHb[1] + hi
        gX = gFinal + A @ gS + torch.cat([au, ai])
    eu, gWu = close64(E0[:U], Wu, gHb[0], dtype)
    ei, gWi = close64(E0[U:], Wi, gHb[1], dtype)
    return losses.detach(), (gX + torch.cat([eu, ei]) + rE0, gWu + rWu, gWi + rWi)
