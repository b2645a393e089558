"""MixRec (Zhang et al., WWW'25) stated once more, in plain torch with autograd and (by default) float64: what
tests/test_gpu_mixrec.py holds idgrec_amd/csrc/idg_mixnce.hip, ops.mix_nce, MixrecEngine and the plugin against, and what
tests/test_mixrec_host.py pins to the reference's own numbers (tests/golden/mixrec_small.npz on graph_small.npz's graph)
without a GPU.  Nothing of the library, and nothing of the reference, is imported here.

    X = sum_{l=1..K} A^l E0                     (the sum, not the mean; the ego layer is left out)
    u = X[users],  p = X[U + pos],  n = X[U + neg]
    losses = [ item_beta BPR(u, p, n),  (1 - item_beta) rect(u, p, Mn),  reg_lambda reg(ego rows),
               ssl_lambda (side(u, user_perm, user_beta) + side(p, item_perm, item_beta)) ]

`side` and `rect` are the COLLAPSED forms (include/idgrec.h, idg_mix_nce_f32): with h = normalize(x), mh = normalize(sum_j
nu_j x_j), ch = normalize(beta x + (1 - beta) x[pi]),
    D_i  = sum_j exp(h_i.h_j / T) + exp(h_i.mh / T)
    side = mean_i [ -beta log(exp(ch_i.h_i / T) / D_i + 1e-7) - (1 - beta) log(exp(ch_i.h_pi(i) / T) / D_pi(i) + 1e-7) ]
`side_composed` / `rect_composed` spell the same terms out call by call — four InfoNCE-against-a-set evaluations per step,
each with its own [B, B + 1] matrix — which is the float32 yardstick of the GPU tests and what the collapsed form is held
against in float64 (tests/test_mixrec_host.py).

The five host draws of a step (user_beta, item_beta, nu, user_perm, item_perm) are INPUTS of every function here."""
import torch
import torch.nn.functional as F

from tests.egcf_ref64 import FLOOR, adam64, band, dense_operator, deterministic, errors  # noqa: F401

GUARD = 10e-8


def _hat(x):
    return F.normalize(x, dim=1, eps=1e-12)


def side64(x, perm, beta, nu, t):
    """The collapsed side term of rows x [B, d] (any dtype; differentiable)."""
    h, mh = _hat(x), _hat((nu.to(x.dtype)[:, None] * x).sum(dim=0, keepdim=True))
    ch = _hat(beta * x + (1 - beta) * x[perm])
    D = torch.exp(h @ h.t() / t).sum(dim=1) + torch.exp((h * mh).sum(dim=1) / t)
    first = -torch.log(torch.exp((ch * h).sum(dim=1) / t) / D + GUARD)
    second = -torch.log(torch.exp((ch * h[perm]).sum(dim=1) / t) / D[perm] + GUARD)
    return torch.mean(beta * first + (1 - beta) * second)


def rect64(u, p, n, perm, beta):
    """mean_i -log(exp(hat(u)_i.hat(p)_i) / sum_j exp(hat(u)_i.hat(Mn)_j) + 1e-7), Mn = beta n + (1 - beta) n[perm]."""
    a, ph, s = _hat(u), _hat(p), _hat(beta * n + (1 - beta) * n[perm])
    return torch.mean(-torch.log(torch.exp((a * ph).sum(dim=1)) / torch.exp(a @ s.t()).sum(dim=1) + GUARD))


def nce_all(e1, e2, e2_all, t):
    """InfoNCE of anchors e1 with positives e2 against the set e2_all (which need not hold e2): rows normalised, the
    1e-7 guard inside the log, the mean over the anchors."""
    e1, e2, e2_all = _hat(e1), _hat(e2), _hat(e2_all)
    pos = torch.exp((e1 * e2).sum(dim=-1) / t)
    ttl = torch.exp(e1 @ e2_all.t() / t).sum(dim=1)
    return torch.mean(-torch.log(pos / ttl + GUARD))


def side_composed(x, perm, beta, nu, t):
    m = (nu.to(x.dtype)[:, None] * x).sum(dim=0, keepdim=True)
    x2 = x[perm]
    c = beta * x + (1 - beta) * x2
    return beta * nce_all(x, c, torch.cat([x2, m]), t) + (1 - beta) * nce_all(x2, c, torch.cat([x, m]), t)


def rect_composed(u, p, n, perm, beta):
    return nce_all(u, p, beta * n + (1 - beta) * n[perm], 1.0)


def mix_terms(u, p, n, draws, t, ssl_weight, composed=False):
    """(loss[0], loss[1]) of idg_mix_nce_f32 on gathered rows: (1 - item_beta) rect, ssl_weight (side_u + side_p)."""
    ub, ib, nu, up, ip = draws
    side, rect = (side_composed, rect_composed) if composed else (side64, rect64)
    return (1 - ib) * rect(u, p, n, ip, ib), ssl_weight * (side(u, up, ub, nu, t) + side(p, ip, ib, nu, t))


def panel_terms(panel, U, users, pos, neg, draws, t, ssl_weight, dtype=torch.float64, upstream=None, composed=False):
    """The two terms on panel rows and the gradient of up[0] loss[0] + up[1] loss[1] w.r.t. the panel."""
    X = panel.detach().to(dtype).clone().requires_grad_(True)
    ub, ib, nu, up, ip = draws
    draws = (float(ub), float(ib), nu.to(dtype), up.long(), ip.long())
    with deterministic():
        l0, l1 = mix_terms(X[users.long()], X[U + pos.long()], X[U + neg.long()], draws, t, ssl_weight, composed)
        w = (1.0, 1.0) if upstream is None else upstream
        (g,) = torch.autograd.grad(w[0] * l0 + w[1] * l1, X)
    return torch.stack([l0, l1]).detach(), g


def propagate64(A, E0, K):
    x, total = E0, None
    for _ in range(K):
        x = A @ x
        total = x if total is None else total + x
    return total


def step64(A, E0, users, pos, neg, draws, K, reg_lambda, ssl_lambda, t, num_users, dtype=torch.float64, composed=False):
    """MixRec's forward and backward on a dense operator A [n, n].  E0: the [n, d] ego panel, users first; draws: (user_beta,
    item_beta, nu [B], user_perm [B], item_perm [B]).  Returns (losses [4], d sum(losses) / d E0, X)."""
    U = int(num_users)
    A = A.to(dtype)
    E0 = E0.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = users.long(), pos.long(), neg.long()
    ub, ib, nu, up, ip = draws
    draws = (float(ub), float(ib), nu.to(dtype), up.long(), ip.long())
    with deterministic():
        X = propagate64(A, E0, K)
        u, p, n = X[users], X[U + pos], X[U + neg]
        x = (u * p).sum(dim=1) - (u * n).sum(dim=1)
        bpr = float(ib) * torch.mean(-torch.log(torch.sigmoid(x) + GUARD))
        blocks = (E0[users], E0[U + pos], E0[U + neg])
        reg = reg_lambda * sum(1 / 2 * blk.norm(2).pow(2) / float(blk.shape[0]) for blk in blocks)
        t2, ssl = mix_terms(u, p, n, draws, t, ssl_lambda, composed)
        (g,) = torch.autograd.grad(bpr + t2 + reg + ssl, E0)
    return torch.stack([bpr, t2, reg, ssl]).detach(), g, X.detach()
