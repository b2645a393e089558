"""The float64 statement of LightGCL's training loss (Cai et al. ICLR'23; the reference's models/LightGCL.py:58-124) in the
COLLAPSED form the kernels of csrc/idg_svdnce.hip implement, in plain torch on the CPU — what tests/test_gpu_lightgcl.py holds
the kernels, the operators, the engine and the plugin against, and what tests/test_lightgcl_host.py pins to the reference's own
float64 run (tests/golden/lightgcl_small.npz).

    E^l = G E^(l-1),   F = sum_{l <= K} E^l,   T = sum_{l < K} E^l = F - E^K          (G the symmetric normalised adjacency)
    P_i = V^T T_i,  P_u = U^T T_u                                                      (two [q, d] projections)
    view rows:  G_u = E_u^0 + (U S) P_i,   G_i = E_i^0 + (V S) P_u                     (only the batch's rows are formed)
    side(g, F_side, ids) = ( mean_b lse_b,  mean_b clamp(<F_ids[b], g_b> / tau, -5, 5) )
    lse_b = log(sum_j exp(s_bj) + 1e-8),  s_bj = <g_b, F_j> / tau
and the log-sum-exp is evaluated with the true running maximum, m_b + log(sum_j exp(s_bj - m_b) + 1e-8 exp(-m_b)): finite where
exp(s) overflows, and still log(1e-8 + ..) where every score is far below zero.

`layered=True` evaluates the reference's own layer-by-layer expressions instead (torch.exp of the raw scores and all): the
yardstick composition, in float64 to prove the collapse identity and in float32 to measure what an fp32 evaluation with
another summation order costs."""
import math

import numpy as np
import torch

GUARD = 1e-8


def dense_operator(indptr, indices, data, shape, dtype=torch.float64):
    """The CSR adjacency as a dense matrix (the `small` inputs: 550 x 550)."""
    A = np.zeros(shape, dtype=np.float64)
    for r in range(shape[0]):
        A[r, indices[indptr[r]:indptr[r + 1]]] = data[indptr[r]:indptr[r + 1]]
    return torch.from_numpy(A).to(dtype)


def symmetric_operator(indptr, indices, data, U, I, dtype=torch.float64):
    """[[0, R], [R^T, 0]] dense from the CSR arrays of the rectangular R [U, I] (the fixture's R_* arrays)."""
    R = dense_operator(indptr, indices, data, (U, I), dtype)
    A = torch.zeros((U + I, U + I), dtype=dtype)
    A[:U, U:], A[U:, :U] = R, R.t()
    return A


def lse_guarded(s):
    """log(sum_j exp(s_bj) + 1e-8) per row with the running maximum; s [B, N].  m + log(S + 1e-8 exp(-m)) with the inner
    logarithm as logaddexp(log S, log 1e-8 - m), so that exp(-m) is never formed (it overflows for m below -709)."""
    m = s.max(dim=1, keepdim=True).values
    S = torch.exp(s - m).sum(dim=1, keepdim=True)
    return (m + torch.logaddexp(torch.log(S), math.log(GUARD) - m)).squeeze(1)


def side_terms(g, table, ids, tau, naive=False):
    """(mean lse, mean clamped positive) of one side: g [B, d] the view rows, table [N, d] the side's final rows."""
    s = g @ table.t() / tau
    lse = torch.log(torch.exp(s).sum(1) + GUARD) if naive else lse_guarded(s)
    pos = torch.clamp((table[ids] * g).sum(1) / tau, -5.0, 5.0)
    return lse.mean(), pos.mean()


def positives(g, table, ids, tau):
    """The unclamped positive scores."""
    return (table[ids] * g).sum(1) / tau


def propagate(A, E0, K):
    """(F, E^K): the layer sum 0 .. K and the last layer."""
    cur, total = E0, E0
    for _ in range(K):
        cur = A @ cur
        total = total + cur
    return total, cur


def views_collapsed(A, E0, svd_u, s, svd_v, K, U, users, pos):
    """(F, g_u [B, d], g_i [B, d]) by the collapse identity."""
    F, EK = propagate(A, E0, K)
    T = F - EK
    P_i, P_u = svd_v.t() @ T[U:], svd_u.t() @ T[:U]
    g_u = E0[:U][users] + (svd_u * s)[users] @ P_i
    g_i = E0[U:][pos] + (svd_v * s)[pos] @ P_u
    return F, g_u, g_i


def views_layered(A, E0, svd_u, s, svd_v, K, U, users, pos):
    """(F, g_u, g_i) as the reference writes them: per layer, over all rows, then summed and gathered."""
    R = A[:U, U:]
    u_mul_s, v_mul_s = svd_u @ torch.diag(s), svd_v @ torch.diag(s)
    eu, ei = [E0[:U]], [E0[U:]]
    gu, gi = [E0[:U]], [E0[U:]]
    for l in range(1, K + 1):
        zu, zi = R @ ei[l - 1], R.t() @ eu[l - 1]
        gu.append(u_mul_s @ (svd_v.t() @ ei[l - 1]))
        gi.append(v_mul_s @ (svd_u.t() @ eu[l - 1]))
        eu.append(zu)
        ei.append(zi)
    F = torch.cat([torch.stack(eu, 1).sum(1), torch.stack(ei, 1).sum(1)])
    return F, torch.stack(gu, 1).sum(1)[users], torch.stack(gi, 1).sum(1)[pos]


def step64(A, E0, svd_u, s, svd_v, users, pos, neg, K, reg_lambda, ssl_lambda, tau, U, dtype=torch.float64, layered=False):
    """One forward + backward.  Returns (losses [bpr, reg_lambda reg, ssl], d sum / d E0 [n, d], F, parts) with
    parts = [lse_u, pos_u, lse_i, pos_i] (the four raw terms) — everything in `dtype`."""
    A, svd_u, s, svd_v = (t.to(dtype) for t in (A, svd_u, s, svd_v))
    E0 = E0.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = users.long(), pos.long(), neg.long()
    F, g_u, g_i = (views_layered if layered else views_collapsed)(A, E0, svd_u, s, svd_v, K, U, users, pos)
    ue, pe, ne = F[:U][users], F[U:][pos], F[U:][neg]
    bpr = (-torch.log(torch.sigmoid((ue * pe).sum(1) - (ue * ne).sum(1)) + 10e-8)).mean()  # losses.get_bpr_loss
    u0, p0, n0 = E0[:U][users], E0[U:][pos], E0[U:][neg]
    reg = reg_lambda * 0.5 * (u0.pow(2).sum() + p0.pow(2).sum() + n0.pow(2).sum()) / float(users.shape[0])
    lse_u, pos_u = side_terms(g_u, F[:U], users, tau, naive=layered)
    lse_i, pos_i = side_terms(g_i, F[U:], pos, tau, naive=layered)
    ssl = ssl_lambda * (-(pos_u + pos_i) + (lse_u + lse_i))
    losses = torch.stack([bpr, reg, ssl])
    (grad,) = torch.autograd.grad(losses.sum(), E0)
    parts = torch.stack([lse_u, pos_u, lse_i, pos_i]).detach()
    return losses.detach(), grad, F.detach(), parts


def adam_steps(A, E0, svd_u, s, svd_v, batches, K, reg_lambda, ssl_lambda, tau, U, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update written out, one step per batch: (losses [steps, 3], the panel after each step)."""
    E = E0.detach().double().clone()
    m, v = torch.zeros_like(E), torch.zeros_like(E)
    losses, panels = [], []
    for t, b in enumerate(batches, 1):
        l, g, _, _ = step64(A, E, svd_u, s, svd_v, b[:, 0], b[:, 1], b[:, 2], K, reg_lambda, ssl_lambda, tau, U)
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        E = E - lr / (1 - betas[0] ** t) * m / ((v / (1 - betas[1] ** t)).sqrt() + eps)
        losses.append(l)
        panels.append(E.clone())
    return torch.stack(losses), panels


# ---- the raw call of one side, as idg_svd_nce_f32 states it (tests of the kernel alone)
def svd_nce64(final_panel, ego_panel, row0, N, AS, P, ids, tau, upstream=(1.0, 1.0), dtype=torch.float64, naive=False):
    """(loss [2], g_final [n, d], g_ego [n, d], dP [q, d], positives [B], terms [2, B]) of up[0] loss[0] + up[1] loss[1];
    terms: the per-row summands (log-sum-exp, clamped positive) whose means the two losses are."""
    Fp = final_panel.detach().to(dtype).clone().requires_grad_(True)
    Ep = ego_panel.detach().to(dtype).clone().requires_grad_(True)
    Pp = P.detach().to(dtype).clone().requires_grad_(True)
    AS, ids = AS.to(dtype), ids.long()
    g = Ep[row0:row0 + N][ids] + AS[ids] @ Pp
    table = Fp[row0:row0 + N]
    lse, pos = side_terms(g, table, ids, tau, naive=naive)
    gF, gE, dP = torch.autograd.grad(upstream[0] * lse + upstream[1] * pos, (Fp, Ep, Pp))
    raw = positives(g, table, ids, tau).detach()
    terms = torch.stack([lse_guarded((g @ table.t() / tau).detach().double()), torch.clamp(raw.double(), -5.0, 5.0)])
    return torch.stack([lse, pos]).detach(), gF, gE, dP, raw, terms
