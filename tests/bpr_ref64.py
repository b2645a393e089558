"""The BPR loss pair with its two gradients, and the row-masked Adam step, stated once more in plain torch and (by
default) float64: what tests/test_gpu_bpr.py holds the kernels of idgrec_amd/csrc/idg_bpr.hip against, and what
tests/test_bpr_ref.py pins to the reference's own numbers (tests/golden/graph_small.npz, graph_tiny.npz, next_small.npz)
without a GPU.  Nothing of the library is imported here.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick of egcf_ref64.band()."""
import torch

from tests.egcf_ref64 import FLOOR, adam64, band, deterministic, errors  # noqa: F401  (one rule, one set of helpers)


def bpr64(fin, ego, U, users, pos, neg, reg_lambda, reg_users=True, dtype=torch.float64, upstream=None):
    """utility_function/losses.py: get_bpr_loss on the final panel's rows and reg_lambda * get_reg_loss on the ego panel's.

      losses[0] = mean_i( -log( sigmoid(<f_u, f_p> - <f_u, f_n>) + 10e-8 ) )
      losses[1] = reg_lambda * sum over blocks of  1/2 * || ego[rows of the block] ||_2^2 / B
    with the blocks (users, U + pos, U + neg), or the two item blocks only when reg_users is false (models/NGCF.py,
    models/EGCF.py).  fin: [n, d_final], ego: [n, d_ego], users first; the widths may differ.

    Returns (losses [2], d losses[0] / d fin, d losses[1] / d ego) in `dtype`; with upstream = (a, b) the two gradients are
    those of a * losses[0] and b * losses[1] (the losses themselves are returned unscaled).  `fin is ego` (MFBPR): one
    panel receives the sum of both gradients, returned in both places."""
    same = fin is ego
    f = fin.detach().to(dtype).clone().requires_grad_(True)
    e = f if same else ego.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = users.long(), U + pos.long(), U + neg.long()
    a, b = (1.0, 1.0) if upstream is None else (float(upstream[0]), float(upstream[1]))
    with deterministic():
        fu, fp, fn = f[users], f[pos], f[neg]
        x = (fu * fp).sum(dim=1) - (fu * fn).sum(dim=1)
        bpr = torch.mean(-torch.log(torch.sigmoid(x) + 10e-8))
        blocks = (e[users], e[pos], e[neg]) if reg_users else (e[pos], e[neg])
        reg = reg_lambda * sum(1 / 2 * blk.norm(2).pow(2) / float(blk.shape[0]) for blk in blocks)
        total = a * bpr + b * reg
        if same:
            (g,) = torch.autograd.grad(total, f)
            gf = ge = g
        else:
            gf, ge = torch.autograd.grad(total, (f, e))
    return torch.stack([bpr, reg]).detach(), gf, ge


def masked(g, bits):
    """g with the rows whose entry of the bool vector `bits` is clear set to zero: what idg_adam_rows_f32 reads."""
    return torch.where(bits[:, None], g, torch.zeros((), dtype=g.dtype, device=g.device))


def adam_rows64(W, g_list, bits_list, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """adam64 on [n, d] tables where step k reads the gradient at the rows flagged in bits_list[k] (bool [n]) only and
    G = 0 elsewhere: an unflagged row's moments still decay and its parameters still move by them.  What the unflagged
    rows of g_list[k] hold (NaN included) is never used."""
    return adam64(W, [masked(g.detach().to(dtype), b) for g, b in zip(g_list, bits_list)], lr=lr, betas=betas, eps=eps,
                  dtype=dtype)
