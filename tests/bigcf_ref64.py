"""BIGCF's intent layer (Zhang et al., SIGIR'24), its gradients, its five InfoNCE terms and its training step stated once
more, in plain torch and (by default) float64: what tests/test_gpu_bigcf.py holds the kernels of
idgrec_amd/csrc/idg_intent.hip, ops.intent_mix and the plugin against, and what tests/test_bigcf_host.py pins to the
reference's own numbers (tests/golden/bigcf_small.npz on graph_small.npz's graph) without a GPU.  Nothing of the library is
imported here.

    X = sum_{l=1..K} A^l E0            (the sum, not the mean; the ego layer is left out)
    S = X @ W,  P = softmax(S, dim=1),  T = P @ W^T,  F = X + T * Z       W = W_u on the user rows, W_i on the item rows

Z, the reference's torch.randn_like panel, is an INPUT of every function here.  The layer's gradients have a closed form
(intent_grads64), which tests/test_bigcf_host.py holds against float64 autograd.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick of egcf_ref64.band()."""
import torch

from tests.egcf_ref64 import FLOOR, adam64, band, dense_operator, deterministic, errors, infonce64  # noqa: F401


def intent64(X, W, Z, dtype=torch.float64):
    """(F, T) of one block of rows.  Differentiable in whatever requires a gradient."""
    X, W = X.to(dtype), W.to(dtype)
    T = torch.softmax(X @ W, dim=1) @ W.t()
    return X + T * Z.to(dtype), T


def _flags(rows, n, device):
    """bool [n] from None (all rows), a bool vector, or a list of row numbers."""
    if rows is None:
        return torch.ones(n, dtype=torch.bool, device=device)
    rows = torch.as_tensor(rows, device=device)
    if rows.dtype == torch.bool:
        return rows
    out = torch.zeros(n, dtype=torch.bool, device=device)
    out[rows.long()] = True
    return out


def intent_grads64(X, W, Z, gF, gT_in, rows=None, dtype=torch.float64):
    """The closed form at the flagged rows (what gF, gT_in, X and Z hold off them, NaN included, is not used):
        gT = (gT_in or 0) + gF * Z;  gP = gT @ W;  gS = P * (gP - rowsum(P * gP));  gX = gF + gS @ W^T;
        gW = X^T @ gS + gT^T @ P.
    Returns (gX with zero rows off the flags, gW)."""
    n = X.shape[0]
    fl = _flags(rows, n, X.device)[:, None]
    zero = torch.zeros((), dtype=dtype, device=X.device)
    X, W = torch.where(fl, X.to(dtype), zero), W.to(dtype)
    gF = torch.where(fl, gF.to(dtype), zero)
    gT = gF * torch.where(fl, Z.to(dtype), zero)
    if gT_in is not None:
        gT = gT + torch.where(fl, gT_in.to(dtype), zero)
    P = torch.softmax(X @ W, dim=1)
    gP = gT @ W
    gS = P * (gP - (P * gP).sum(dim=1, keepdim=True))
    gX = torch.where(fl, gF + gS @ W.t(), zero)
    return gX, X.t() @ gS + gT.t() @ P


def propagate64(A, E0, K):
    x, total = E0, None
    for _ in range(K):
        x = A @ x
        total = x if total is None else total + x
    return total


def step64(A, E0, Wu, Wi, users, pos, neg, Z, K, reg_lambda, ssl_lambda, t, num_users, dtype=torch.float64):
    """BIGCF.forward (models/BIGCF.py:46-106) and its backward on a dense operator A [n, n].  E0: the [n, d] ego panel, users
    first; Wu, Wi: the [d, k] intent matrices; Z: the [n, d] noise panel.
    Returns (losses [3] = [bpr, reg_lambda * reg, ssl_lambda * (uu + pp + up + uu' + pp')], the five InfoNCE terms [5],
    (d sum(losses) / d E0, / d Wu, / d Wi), F, T)."""
    U = int(num_users)
    A = A.to(dtype)
    E0, Wu, Wi = (x.detach().to(dtype).clone().requires_grad_(True) for x in (E0, Wu, Wi))
    users, pos, neg = users.long(), pos.long(), neg.long()
    Z = Z.to(dtype)
    with deterministic():
        X = propagate64(A, E0, K)
        Fu, Tu = intent64(X[:U], Wu, Z[:U], dtype)
        Fi, Ti = intent64(X[U:], Wi, Z[U:], dtype)
        ue, pe, ne = Fu[users], Fi[pos], Fi[neg]
        x = (ue * pe).sum(dim=1) - (ue * ne).sum(dim=1)
        bpr = torch.mean(-torch.log(torch.sigmoid(x) + 10e-8))
        blocks = (E0[users], E0[U + pos], E0[U + neg], Wu, Wi)
        reg = reg_lambda * sum(1 / 2 * blk.norm(2).pow(2) / float(blk.shape[0]) for blk in blocks)
        terms = torch.stack([infonce64(ue, ue, t, dtype), infonce64(pe, pe, t, dtype), infonce64(ue, pe, t, dtype),
                             infonce64(Tu[users], Tu[users], t, dtype), infonce64(Ti[pos], Ti[pos], t, dtype)])
        ssl = ssl_lambda * terms.sum()
        grads = torch.autograd.grad(bpr + reg + ssl, (E0, Wu, Wi))
    return (torch.stack([bpr, reg, ssl]).detach(), terms.detach(), grads, torch.cat([Fu, Fi]).detach(),
            torch.cat([Tu, Ti]).detach())
