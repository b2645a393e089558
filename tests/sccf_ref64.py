"""SCCF (Wu et al., KDD'24) stated once more, in plain torch with autograd and (by default) float64: what
tests/test_gpu_sccf.py holds idgrec_amd/csrc/idg_sccf.hip, ops.sccf_loss, the engine hook and the plugin against, and what
tests/test_sccf_host.py pins to the reference's own numbers (tests/golden/sccf_small.npz on graph_small.npz's graph) without
a GPU.  Nothing of the library, and nothing of the reference, is imported here.

    X = E0 (encoder MF)  or  mean_{k=0..K} A^k E0 (any other encoder)
    a_i = normalize(X[users[i]]),  b_i = normalize(X[U + pos[i]]),  f(s) = exp(s / T) + exp(s^2 / T)
    losses = [ -mean_i log f(a_i.b_i),  log(mean over [Nu, Ni] of f(ah_k.bh_l) cu_k ci_l) ]

The second term in two forms: `literal` — torch.unique, the [Nu, Ni] matrix of the distinct rows and the outer product of
their multiplicities, as the reference spells it — and `collapsed` — log(sum_{i<B} sum_{j<B} f(a_i.b_j) / (Nu Ni)), which is
what the kernel computes (cu_k ci_l counts the occurrences of the pair in B x B).  The float32 evaluation of the LITERAL
form is the yardstick of the GPU tests: how far a correct float32 evaluation sits from the float64 statement."""
import torch
import torch.nn.functional as F

from tests.egcf_ref64 import adam64, dense_operator, deterministic, errors  # noqa: F401


def _hat(x):
    return F.normalize(x, dim=-1)


def _f(s, t):
    return (s / t).exp() + (s ** 2 / t).exp()


def up64(a_rows, b_rows, t):
    """-mean_i log f(a_i.b_i) of the gathered rows (any dtype; differentiable)."""
    ip = (_hat(a_rows) * _hat(b_rows)).sum(dim=1)
    return -_f(ip, t).log().mean()


def down_literal(X, U, users, pos, t):
    """The reference's form: unique ids, their rows, the [Nu, Ni] score matrix weighted by the multiplicities."""
    u_idx, u_counts = torch.unique(users, return_counts=True)
    i_idx, i_counts = torch.unique(pos, return_counts=True)
    cu, ci = u_counts.reshape(-1, 1).to(X.dtype), i_counts.reshape(-1, 1).to(X.dtype)
    sim = _hat(X[u_idx]) @ _hat(X[U + i_idx]).T
    return (_f(sim, t) * (cu @ ci.T)).mean().log()


def down_collapsed(X, U, users, pos, t):
    """The same number over the batch rows as they come: sum over B x B, divided by the two distinct-id counts."""
    nu, ni = int(torch.unique(users).numel()), int(torch.unique(pos).numel())
    sim = _hat(X[users]) @ _hat(X[U + pos]).T
    return (_f(sim, t).sum() / (nu * ni)).log()


def panel_terms(panel, U, users, pos, t, dtype=torch.float64, upstream=None, collapsed=False):
    """(losses [2], d(up[0] loss[0] + up[1] loss[1]) / d panel) on the rows of an [n, d] panel."""
    X = panel.detach().to(dtype).clone().requires_grad_(True)
    users, pos = users.long(), pos.long()
    down = down_collapsed if collapsed else down_literal
    with deterministic():
        l0, l1 = up64(X[users], X[U + pos], t), down(X, U, users, pos, t)
        w = (1.0, 1.0) if upstream is None else upstream
        (g,) = torch.autograd.grad(w[0] * l0 + w[1] * l1, X)
    return torch.stack([l0, l1]).detach(), g


def propagate64(A, E0, K):
    x, total = E0, E0
    for _ in range(K):
        x = A @ x
        total = total + x
    return total / (K + 1)


def step64(A, E0, users, pos, layers, t, num_users, dtype=torch.float64, collapsed=False):
    """SCCF's forward and backward.  A: the dense [n, n] operator, or None for the MF encoder (layers is then ignored); E0:
    the [n, d] ego panel, users first.  Returns (losses [2], d sum(losses) / d E0, X)."""
    U = int(num_users)
    E0 = E0.detach().to(dtype).clone().requires_grad_(True)
    users, pos = users.long(), pos.long()
    down = down_collapsed if collapsed else down_literal
    with deterministic():
        X = E0 if A is None else propagate64(A.to(dtype), E0, layers)
        l0, l1 = up64(X[users], X[U + pos], t), down(X, U, users, pos, t)
        (g,) = torch.autograd.grad(l0 + l1, E0)
    return torch.stack([l0, l1]).detach(), g, X.detach()


def case_inputs(B, d, seed, U=45, I=61, device="cpu", form="random"):
    """The inputs of one case of the GPU tests' grid, drawn on the CPU (the same numbers on either side): the panel
    [U + I, d] and the id lists.  form: `random` (B >= U or I repeats ids), `distinct` (U = I = B rows, a permutation
    each), `one_user` (one user B times), `zero_rows` (`random` with two panel rows zeroed)."""
    gen = torch.Generator().manual_seed(seed)
    if form == "distinct":
        U = I = B
    panel = torch.randn(U + I, d, generator=gen, dtype=torch.float32) * 0.3
    if form == "distinct":
        users, pos = torch.randperm(B, generator=gen), torch.randperm(B, generator=gen)
    else:
        users = torch.randint(0, U, (B,), generator=gen)
        pos = torch.randint(0, I, (B,), generator=gen)
        if form == "one_user":
            users = torch.full((B,), int(users[0]), dtype=torch.int64)
        if form == "zero_rows":  # a zero panel row as user and as positive (zero_rows_of names them)
            panel[int(users[2])] = 0
            panel[U + int(pos[5])] = 0
    return panel.to(device), users.to(device), pos.to(device), U


GRID_B = (1, 96, 127, 128, 129, 257)
GRID_D = (48, 64, 100, 256)
GRID_T = (0.1, 1.0)


def grid_seed(B, d, t):
    return B * 1000 + d + (7 if t == 1.0 else 0)


def grid_upstream(B):
    """The incoming gradient pair of a grid case: (0.7, -1.3) at B = 1 (where the unit pair's two terms cancel: -log f + log f)
    and at B = 129, ones elsewhere."""
    return (0.7, -1.3) if B in (1, 129) else None


# the cases over every built width (tests/widths.py: EVERY_NDT): (B, d) at WIDTH_T, the upstream pair of grid_upstream(B)
WIDTH_B = (129, 257)
WIDTH_T = 0.1


def width_seed(B, d):
    """Apart from every seed of the grid (below 258000) and of the riders (below 8300)."""
    return 500000 + B * 1000 + d


def zero_rows_of(users, pos, U):
    return (int(users[2]), U + int(pos[5]))


# the cases that ride on a few sizes of grid (a): (form, B, d, T, seed)
RIDERS = tuple((form, B, d, t, 31 * B + d) for form in ("distinct", "one_user") for B, d, t in ((96, 64, 0.1), (129, 48, 1.0), (257, 100, 0.1))) \
    + tuple(("zero_rows", B, d, t, 17 * B + d) for B, d, t in ((129, 64, 0.1), (96, 100, 1.0))) \
    + tuple(("random", B, d, t, 13 * B + d) for B, d, t in ((127, 64, 0.1), (257, 48, 1.0)))
