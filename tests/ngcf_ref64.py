"""NGCF's layer and training step stated once more, in plain torch / numpy and (by default) float64: what
tests/test_gpu_ngcf.py holds the kernels of idgrec_amd/csrc/idg_ngcf.hip and idg_dense.hip and the fused chain of
idgrec_amd/ngcf.py against, and what tests/test_ngcf_ref.py pins to the reference's own numbers (tests/golden/next_small.npz
on graph_small.npz) without a GPU.  Nothing of the library is imported here.

The message-dropout mask is a PUBLISHED function of (seed, stream, row, feature) (idgrec_amd/csrc/idg_dropout.h):
mix64 / keep_mask restate it in numpy uint64, so that kernel and reference share one mask the way dense_operator makes them
share one graph.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick of egcf_ref64.band()."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.bpr_ref64 import bpr64
from tests.egcf_ref64 import FLOOR, adam64, band, dense_operator, deterministic, errors  # noqa: F401  (one rule, one set of helpers)

_M64 = (1 << 64) - 1
_GOLDEN, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix64(seed, stream, rows, f4):
    """The splitmix64 finaliser of z = seed + GOLDEN (stream + 1) + row MUL1 + (feature >> 2) MUL2, everything modulo 2^64.
    rows, f4: integers or integer arrays (broadcast against each other); returns numpy uint64."""
    base = np.uint64((int(seed) + _GOLDEN * (int(stream) + 1)) & _M64)
    rows, f4 = np.asarray(rows).astype(np.uint64), np.asarray(f4).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = base + rows * np.uint64(_MUL1) + f4 * np.uint64(_MUL2)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)
        return z ^ (z >> np.uint64(31))


def keep_scale(p):
    """float32(1) / (float32(1) - float32(p)): rounded in float32 FIRST, whatever the dtype it is used in afterwards."""
    return float(np.float32(1) / (np.float32(1) - np.float32(p)))


def keep_mask(p, seed, stream, n, d, dtype=torch.float64):
    """[n, d]: keep_scale(p) where element (row, f) is kept, 0 where it is dropped.  Feature f reads bits 16 (f & 3) .. + 15 of
    mix64(seed, stream, row, f >> 2); it is kept iff float32(bits) * 2^-16 >= float32(p).  p <= 0: all ones."""
    if p <= 0:
        return torch.ones((n, d), dtype=dtype)
    f = np.arange(d, dtype=np.int64)
    z = mix64(seed, stream, np.arange(n, dtype=np.int64)[:, None], (f >> 2)[None, :])
    bits = (z >> (np.uint64(16) * (f & 3).astype(np.uint64))[None, :]) & np.uint64(0xFFFF)
    u = bits.astype(np.float32) * np.float32(2.0 ** -16)
    keep = u >= np.float32(p)
    return torch.from_numpy(keep).to(dtype) * keep_scale(p)


def tail64(S1, S2, b1, b2, slope, mask, dtype=torch.float64):
    """models/NGCF.py:88-104 after the two products: t = (S1 + b1) + (S2 + b2) (S2 = None: 0), E = leaky_relu(t) * mask,
    N = F.normalize(E, dim=1, eps=1e-12).  Returns (E, N); differentiable in whatever requires a gradient."""
    t = S1.to(dtype) + b1.to(dtype).reshape(1, -1)
    u = b2.to(dtype).reshape(1, -1)
    if S2 is not None:
        u = S2.to(dtype) + u
    E = F.leaky_relu(t + u, slope) * mask.to(device=t.device, dtype=dtype)
    return E, F.normalize(E, p=2, dim=1, eps=1e-12)


def layer64(side, ego, W1, W2, b1, b2, slope, mask, dtype=torch.float64):
    """One layer (models/NGCF.py:85-106): tail64(side @ W1 + (ego * side) @ W2, None, ...)."""
    side, ego = side.to(dtype), ego.to(dtype)
    return tail64(side @ W1.to(dtype) + (ego * side) @ W2.to(dtype), None, b1, b2, slope, mask, dtype)


def _flags(gn_rows, n, device):
    """bool [n] from None (all rows), a bool vector, or a list of row numbers."""
    if gn_rows is None:
        return torch.ones(n, dtype=torch.bool, device=device)
    gn_rows = torch.as_tensor(gn_rows, device=device)
    if gn_rows.dtype == torch.bool:
        return gn_rows
    out = torch.zeros(n, dtype=torch.bool, device=device)
    out[gn_rows.long()] = True
    return out


def _upstream(E, N, gE, gN, gn_rows, dtype):
    """sum(E * gE) + sum(N * gN at the flagged rows): the scalar whose gradient the backward kernels form.  What gN holds off
    the flagged rows (NaN included) is not used."""
    total = E.new_zeros(())
    if gE is not None:
        total = total + (E * gE.to(dtype)).sum()
    if gN is not None:
        fl = _flags(gn_rows, E.shape[0], E.device)
        total = total + (N * torch.where(fl[:, None], gN.to(dtype), torch.zeros((), dtype=dtype, device=E.device))).sum()
    return total


def tail_grads64(S1, S2, b1, b2, slope, mask, gE, gN, gn_rows=None, dtype=torch.float64):
    """gT = d (sum(E * gE) + sum(N * gN)) / d t by autograd on tail64; gE or gN may be None, gN counts at gn_rows only."""
    S = S1.detach().to(dtype).clone().requires_grad_(True)
    E, N = tail64(S, None if S2 is None else S2.detach(), b1.detach(), b2.detach(), slope, mask, dtype)
    (gT,) = torch.autograd.grad(_upstream(E, N, gE, gN, gn_rows, dtype), S)
    return gT


def layer_grads64(side, ego, W1, W2, b1, b2, slope, mask, gE, gN, gn_rows=None, dtype=torch.float64):
    """Autograd on layer64.  Returns (gT, g_side, g_ego, flat) with flat = [gW1 | gb1 | gW2 | gb2], the layout of
    idg_ngcf_wgrad_f32 / idg_ngcf_layer_bwd_f32."""
    leaf = lambda x: x.detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    side, ego, W1, W2, b1, b2 = (leaf(x) for x in (side, ego, W1, W2, b1, b2))
    S = side @ W1 + (ego * side) @ W2
    E, N = tail64(S, None, b1, b2, slope, mask, dtype)
    gT, gs, ge, gW1, gb1, gW2, gb2 = torch.autograd.grad(_upstream(E, N, gE, gN, gn_rows, dtype), (S, side, ego, W1, b1, W2, b2))
    return gT, gs, ge, torch.cat([gW1.reshape(-1), gb1.reshape(-1), gW2.reshape(-1), gb2.reshape(-1)])


def step64(A, E0, small, users, pos, neg, slope, masks, reg_lambda, num_users, dtype=torch.float64):
    """NGCF.forward (models/NGCF.py:67-130) and its backward on a dense operator A [n, n].  E0: the [n, d] ego panel, users
    first; small: K tuples (W_gcn, b_gcn, W_bi, b_bi); masks: K keep masks [n, d] (None: dropout off).
    final = cat([E0, N_1 .. N_K], dim=1); the loss is bpr64 on final with the item-only regulariser on E0.
    Returns (losses [2] = [bpr, reg_lambda * reg], d sum(losses) / d E0, [K tuples of the small tensors' gradients], final)."""
    A = A.to(dtype)
    E0 = E0.detach().to(dtype).clone().requires_grad_(True)
    small = [tuple(t.detach().to(dtype).clone().requires_grad_(True) for t in layer) for layer in small]
    ego, layers = E0, [E0]
    for l, (wg, bg, wb, bb) in enumerate(small):
        mask = torch.ones((), dtype=dtype, device=E0.device) if masks is None or masks[l] is None else masks[l]
        ego, N = layer64(A @ ego, ego, wg, wb, bg, bb, slope, mask, dtype)
        layers.append(N)
    final = torch.cat(layers, dim=1)
    losses, gf, ge = bpr64(final, E0, num_users, users, pos, neg, reg_lambda, reg_users=False, dtype=dtype)
    flat = [t for layer in small for t in layer]
    grads = torch.autograd.grad(final, [E0] + flat, grad_outputs=gf)
    return losses, grads[0] + ge, [tuple(grads[1 + 4 * l: 5 + 4 * l]) for l in range(len(small))], final.detach()
