"""EGCF's training step stated once more, in plain torch and (by default) float64: what tests/test_gpu_egcf.py holds the
fused HIP chain (idgrec_amd/egcf.py) and its kernels against, and what tests/test_egcf_ref.py pins to the reference's own
numbers (tests/golden/egcf_small.npz) without a GPU.  Nothing of the library is imported here.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick for how far a correct float32 evaluation may sit from the reference (band() below)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 8 * 2.0 ** -24  # a lucky float32 composition must not fail a correct kernel


@contextlib.contextmanager
def deterministic():
    """A gather's backward adds the occurrences of an id with float atomics on a device, in whatever order they arrive:
    inside this block torch takes its ordered form instead, so that the float32 composition — the yardstick — gives the
    same number on every run."""
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


def dense_operator(indptr, indices, values, shape, dtype=torch.float64, device="cpu"):
    """The CSR operator an ops.Graph handle receives, as a dense matrix: the values rounded to float32 first (what the
    handle stores), then cast up, so kernel and reference share one operator."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    vals = np.asarray(values).astype(np.float32)
    rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(indptr))
    M = torch.zeros(shape, dtype=dtype)
    M.index_put_((torch.from_numpy(rows), torch.from_numpy(indices)), torch.from_numpy(vals).to(dtype), accumulate=True)
    return M.to(device)


def infonce64(a, b, t, dtype=torch.float64):
    """losses.get_InfoNCE_loss: rows normalised with F.normalize's eps = 1e-12, the 10e-6 guard inside the log."""
    a, b = F.normalize(a.to(dtype), dim=1, eps=1e-12), F.normalize(b.to(dtype), dim=1, eps=1e-12)
    pos = torch.exp((a * b).sum(dim=-1) / t)
    ttl = torch.exp(torch.matmul(a, b.transpose(0, 1)) / t).sum(dim=1)
    return torch.mean(-torch.log(pos / ttl + 10e-6))


def egcf_aggregate64(R, A, E, K, mode):
    """models/EGCF.py: parallel_aggregate / alternating_aggregate on dense operators (R: [U, I]; A: [U + I, U + I], only
    read by `parallel`).  Returns (users, items), each summed over the K layers."""
    U = R.shape[0]
    if mode == "parallel":
        x = torch.cat([torch.tanh(R @ E), E])
        total = None
        for _ in range(K):
            x = torch.tanh(A @ x)
            total = x if total is None else total + x
        return total[:U], total[U:]
    item, users, items = E, None, None
    for _ in range(K):
        user = torch.tanh(R @ item)
        item = torch.tanh(R.t() @ user)
        users = user if users is None else users + user
        items = item if items is None else items + item
    return users, items


def egcf_step64(R, A, E, users, pos, neg, K, mode, reg_lambda, ssl_lambda, t, dtype=torch.float64):
    """EGCF.forward (models/EGCF.py) and its backward: returns (losses [3] = [bpr, reg_lambda * reg, ssl_lambda * (uu + pp +
    up)], d sum(losses) / dE) in `dtype`.  E: the [I, d] item table; users / pos / neg: int64 id lists."""
    R = R.to(dtype)
    A = None if A is None else A.to(dtype)
    E = E.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = users.long(), pos.long(), neg.long()
    with deterministic():
        all_user, all_item = egcf_aggregate64(R, A, E, K, mode)
        ue, pe, ne = all_user[users], all_item[pos], all_item[neg]
        x = (ue * pe).sum(dim=1) - (ue * ne).sum(dim=1)
        bpr = torch.mean(-torch.log(torch.sigmoid(x) + 10e-8))
        reg = sum(1 / 2 * blk.norm(2).pow(2) / float(blk.shape[0]) for blk in (E[pos], E[neg]))
        ssl = infonce64(ue, ue, t, dtype) + infonce64(pe, pe, t, dtype) + infonce64(ue, pe, t, dtype)
        losses = torch.stack([bpr, reg_lambda * reg, ssl_lambda * ssl])
        (dE,) = torch.autograd.grad(losses.sum(), E)
    return losses.detach(), dE


def adam64(W, g_list, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """torch.optim.Adam's recurrence (no weight decay, no amsgrad) from zero moments: the (table, exp_avg, exp_avg_sq)
    after each gradient of g_list, as a list."""
    W = W.detach().to(dtype).clone()
    M, V = torch.zeros_like(W), torch.zeros_like(W)
    out = []
    for step, g in enumerate(g_list, 1):
        g = g.detach().to(dtype)
        M = betas[0] * M + (1 - betas[0]) * g
        V = betas[1] * V + (1 - betas[1]) * g * g
        bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
        W = W - (lr / bc1) * (M / (V.sqrt() / bc2 ** 0.5 + eps))
        out.append((W.clone(), M.clone(), V.clone()))
    return out


def errors(got, ref64, f32, scale=None):
    """(e_kernel, e_f32): max |got - ref64| and max |f32 - ref64| over scale = max |ref64| (or the one given)."""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    dev = ref64.device
    if scale is None:
        scale = float(ref64.abs().max())
    e_k = float((torch.as_tensor(got).to(dev, torch.float64) - ref64).abs().max()) / scale
    e_f = float((torch.as_tensor(f32).to(dev, torch.float64) - ref64).abs().max()) / scale
    return e_k, e_f


def band(e_f32):
    """How far a float32 kernel may sit from the float64 reference: four times the float32 composition's own distance
    (split-K slices, MFMA K order, expf / tanhf versus torch's), floored at 8 * 2^-24."""
    return max(4 * e_f32, FLOOR)
