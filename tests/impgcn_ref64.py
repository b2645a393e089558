"""IMP-GCN's group assignment, propagation and training step stated once more, in plain torch and (by default) float64: what
tests/test_gpu_impgcn.py holds the kernels of idgrec_amd/csrc/idg_group.hip and the fused chain of idgrec_amd/impgcn.py
against, and what tests/test_impgcn_host.py pins to the reference's own numbers (tests/golden/impgcn_small.npz on
graph_small.npz's graph) without a GPU.  Nothing of the library is imported here.

    temp = leaky_relu((E0 + side) @ W_fc^T + b_fc, 0.01) * mask1;  scores = (temp @ W_grp^T + b_grp) * mask2
    member[r] = bitmask of { g : scores[r, g] == max_g scores[r, :] } (users; by value, ties included), every group (items)
    X_g^l = D_g A D_g X_g^(l-1), X_g^0 = E0;  S_l = sum_g X_g^l (groups ascending), S_0 = G E0;  final = mean(S_0 .. S_(L-1))

The masks are ngcf_ref64.keep_mask: the published function of (seed, stream, row, feature) of idgrec_amd/csrc/idg_dropout.h,
the first over (row, feature < 64), the second over (row, g < G).  The membership is a comparison, so no gradient passes
through it: step64 takes it as an INPUT — a near-tie that legitimately flips in float32 cannot poison a whole-step
comparison — and assign64 says which rows are near-tied.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick of egcf_ref64.band()."""
import torch

from tests.bpr_ref64 import bpr64
from tests.egcf_ref64 import FLOOR, adam64, band, dense_operator, errors  # noqa: F401  (one rule, one set of helpers)
from tests.ngcf_ref64 import keep_mask  # noqa: F401

SLOPE = 0.01  # nn.LeakyReLU()
P_DROP = 0.4  # nn.Dropout(p=0.4), hard-coded in the reference
NEAR = 1e-5   # the near-tie rule's factor (the form of test_gpu_gcmc.py's _near_the_kink)


def bits_of(hot):
    """[n, G] bool -> uint8 [n]: bit g set where hot[:, g]."""
    G = hot.shape[1]
    return (hot.to(torch.int64) << torch.arange(G, dtype=torch.int64, device=hot.device)).sum(dim=1).to(torch.uint8)


def groups_of(member, G):
    """uint8 [n] -> [n, G] bool."""
    return ((member.to(torch.int64)[:, None] >> torch.arange(G, dtype=torch.int64, device=member.device)) & 1).bool()


def argmax_set(scores, num_users):
    """The membership of given scores: torch.eq against the top-1 value on the user rows (-0.0 == 0.0), all ones below."""
    hot = torch.eq(scores, scores.max(dim=1, keepdim=True)[0])
    hot[num_users:] = True
    return bits_of(hot)


def assign64(E0, side, W_fc, b_fc, W_grp, b_grp, num_users, mask1=None, mask2=None, dtype=torch.float64):
    """(scores [n, G], member uint8 [n], near bool [n]).  mask1 [n, d] / mask2 [n, G]: keep masks (None: dropout off).  A
    user row is NEAR-tied when some non-maximal score lies within NEAR * max_g(|temp| @ |W_grp|^T + |b_grp|) of the top: a
    correct float32 evaluation may then legitimately choose differently."""
    x = E0.to(dtype) + side.to(dtype)
    temp = torch.nn.functional.leaky_relu(x @ W_fc.to(dtype).t() + b_fc.to(dtype).reshape(1, -1), SLOPE)
    if mask1 is not None:
        temp = temp * mask1.to(device=temp.device, dtype=dtype)
    scores = temp @ W_grp.to(dtype).t() + b_grp.to(dtype).reshape(1, -1)
    if mask2 is not None:
        scores = scores * mask2.to(device=scores.device, dtype=dtype)
    mag = (temp.abs() @ W_grp.to(dtype).abs().t() + b_grp.to(dtype).abs().reshape(1, -1)).max(dim=1, keepdim=True)[0]
    gap = scores.max(dim=1, keepdim=True)[0] - scores
    near = ((gap > 0) & (gap <= NEAR * mag)).any(dim=1)
    near[num_users:] = False
    return scores, argmax_set(scores, num_users), near


def propagate64(A, X0, member, G, n_products, V=None, dtype=torch.float64):
    """The grouped panels of n_products chained products from the shared X0: X_g <- D_g A D_g (X_g + V) (V: a shared addend
    of the input, None: none).  Returns [[X_g^l for g] for l = 1 .. n_products]; differentiable in X0."""
    A = A.to(dtype)
    Dg = groups_of(member, G).to(device=A.device, dtype=dtype)
    X = [X0.to(dtype)] * G
    out = []
    for _ in range(n_products):
        X = [Dg[:, g:g + 1] * (A @ (Dg[:, g:g + 1] * (X[g] if V is None else X[g] + V.to(dtype)))) for g in range(G)]
        out.append(X)
    return out


def final64(A, E0, member, G, L, dtype=torch.float64):
    """models/IMPGCN.py:72-84: the mean of [S_0 = G E0, S_1, .., S_(L-1)], each the sum of its groups in group order."""
    sums = [torch.stack([E0.to(dtype)] * G).sum(0)]
    for X in propagate64(A, E0, member, G, L - 1, dtype=dtype):
        sums.append(torch.stack(X).sum(0))
    return torch.stack(sums, dim=1).mean(dim=1)


def step64(A, E0, member, users, pos, neg, G, L, reg_lambda, num_users, dtype=torch.float64):
    """IMPGCN.forward (models/IMPGCN.py:90-108) and its backward on a dense operator A [n, n] for a GIVEN membership.
    Returns (losses [2] = [bpr, reg_lambda * reg], d sum(losses) / d E0, final, d loss / d final)."""
    E0 = E0.detach().to(dtype).clone().requires_grad_(True)
    final = final64(A, E0, member, G, L, dtype)
    losses, gf, ge = bpr64(final, E0, num_users, users, pos, neg, reg_lambda, reg_users=True, dtype=dtype)
    (g,) = torch.autograd.grad(final, E0, grad_outputs=gf)
    return losses, g + ge, final.detach(), gf
