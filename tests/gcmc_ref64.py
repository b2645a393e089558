"""GCMC's layer, its gradients and its training step stated once more, in plain torch and (by default) float64: what
tests/test_gpu_gcmc.py holds the kernels of idgrec_amd/csrc/idg_gcmc.hip and the fused chain of idgrec_amd/gcmc.py against,
and what tests/test_gcmc_host.py pins to the reference's own numbers (tests/golden/gcmc_small.npz on graph_small.npz's
graph) without a GPU.  Nothing of the library is imported here.

    H = side @ W_gcn + b_gcn;  A = leaky_relu(H, 0.2);  M = A @ W_mlp + b_mlp;  T = keep * M;  N = T / max(|T|_2, 1e-12)
    side_l = Adj @ T_{l-1} (T_0 = E_0),  final = [E_0 | N_1 | .. | N_K]

The gradients are autograd's on these expressions (layer_grads64): torch's leaky_relu backward applies the slope where
H <= 0, torch's normalize has the Jacobian I / eps on a row below the clamp — the conventions of the kernels.  The mask is
ngcf_ref64.keep_mask: the published function of (seed, stream, row, feature) of idgrec_amd/csrc/idg_dropout.h.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick of egcf_ref64.band()."""
import torch

from tests.bpr_ref64 import bpr64
from tests.egcf_ref64 import FLOOR, adam64, band, dense_operator, errors  # noqa: F401  (one rule, one set of helpers)
from tests.gccf_ref64 import _flags
from tests.ngcf_ref64 import keep_mask  # noqa: F401

SLOPE = 0.2
EPS = 1e-12


def hidden64(side, Wg, bg, dtype=torch.float64):
    """H = side @ W_gcn + b_gcn: what LeakyReLU's kink is judged on."""
    return side.to(dtype) @ Wg.to(dtype) + bg.to(dtype).reshape(1, -1)


def layer64(side, Wg, bg, Wm, bm, mask, dtype=torch.float64):
    """(T, N) of one layer, the dropout written as its keep mask (scale where kept, 0 where dropped; a 0-dim one: dropout
    off).  Differentiable in whatever requires a gradient."""
    A = torch.nn.functional.leaky_relu(hidden64(side, Wg, bg, dtype), SLOPE)
    T = (A @ Wm.to(dtype) + bm.to(dtype).reshape(1, -1)) * mask.to(device=side.device, dtype=dtype)
    return T, torch.nn.functional.normalize(T, p=2, dim=1, eps=EPS)


def layer_grads64(side, Wg, bg, Wm, bm, mask, gE, gN, gn_rows=None, dtype=torch.float64):
    """Autograd on layer64 with the upstream gradients gE (of T; None: none) and gN (of N, at the rows of gn_rows only; what
    it holds off them, NaN included, is not used).  Returns (g_side, flat) with flat = [gWg | gbg | gWm | gbm], the layout of
    idg_gcmc_layer_bwd_f32."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (side, Wg, bg, Wm, bm)]
    T, N = layer64(*leaves, mask, dtype=dtype)
    n = side.shape[0]
    zero = torch.zeros((), dtype=dtype, device=side.device)
    up = zero
    if gE is not None:
        up = up + (T * gE.to(dtype)).sum()
    if gN is not None:
        fl = _flags(gn_rows, n, side.device)
        up = up + (N * torch.where(fl[:, None], gN.to(dtype), zero)).sum()
    g = torch.autograd.grad(up, leaves)
    return g[0], torch.cat([t.reshape(-1) for t in g[1:]])


def step64(A, E0, small, users, pos, neg, masks, reg_lambda, num_users, dtype=torch.float64):
    """GCMC.forward (models/GCMC.py:66-116) and its backward on a dense operator A [n, n].  E0: the [n, d] ego panel, users
    first; small: K tuples (W_gcn, b_gcn, W_mlp, b_mlp); masks: K keep masks [n, d] (None: dropout off).
    final = cat([E0, N_1 .. N_K], dim=1); the loss is bpr64 on final with the regulariser on the user, positive and negative
    rows of E0.  Returns (losses [2] = [bpr, reg_lambda * reg], d sum(losses) / d E0, [K tuples of the small tensors'
    gradients], final)."""
    A = A.to(dtype)
    E0 = E0.detach().to(dtype).clone().requires_grad_(True)
    small = [tuple(t.detach().to(dtype).clone().requires_grad_(True) for t in layer) for layer in small]
    ego, layers = E0, [E0]
    for l, (wg, bg, wm, bm) in enumerate(small):
        mask = torch.ones((), dtype=dtype, device=E0.device) if masks is None or masks[l] is None else masks[l]
        ego, norm = layer64(A @ ego, wg, bg, wm, bm, mask, dtype)
        layers.append(norm)
    final = torch.cat(layers, dim=1)
    losses, gf, ge = bpr64(final, E0, num_users, users, pos, neg, reg_lambda, reg_users=True, dtype=dtype)
    flat = [t for layer in small for t in layer]
    grads = torch.autograd.grad(final, [E0] + flat, grad_outputs=gf)
    return losses, grads[0] + ge, [tuple(grads[1 + 4 * l: 5 + 4 * l]) for l in range(len(small))], final.detach()
