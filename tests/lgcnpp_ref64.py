"""float64 torch expressions of LightGCN++'s encoder, written for this project: the row normalisation, its backward J in
closed form (tests/test_lgcnpp_host.py checks it against float64 autograd), the magnitude of J's terms (what a rounding
bound of the fp32 kernel is relative to), and the whole encoder chain (differentiable: its gradients come from autograd).

    y = x / (||x|| + e),    J(t) = (t - y <y, t> (n + e) / n) / (n + e)  for n = ||x|| > 0,    J(t) = t / e  for n == 0
"""
import torch

EPS = 1e-12


def rownorm64(X, eps=EPS):
    """(X / (||X||_2 + eps) per row, the norms), in float64."""
    X = X.double()
    n = X.norm(dim=1)
    return X / (n + eps)[:, None], n


def _coef(Y, T, n, den):
    safe = torch.where(n > 0, n, torch.ones_like(n))
    return torch.where(n > 0, (Y * T).sum(dim=1) * den / safe, torch.zeros_like(n))


def rownorm_bwd64(T, Y, n, eps=EPS, G=None, a=0.0, add2=None):
    """a G + add2 + J(T), J from the normalised rows Y and the norms n, in float64."""
    T, Y, n = T.double(), Y.double(), n.double()
    den = n + eps
    out = (T - Y * _coef(Y, T, n, den)[:, None]) / den[:, None]
    if G is not None:
        out = out + a * G.double()
    if add2 is not None:
        out = out + add2.double()
    return out


def rownorm_bwd_abs64(T, Y, n, eps=EPS, G=None, a=0.0, add2=None):
    """The same expression with every term replaced by its absolute value."""
    T, Y, n = T.double().abs(), Y.double().abs(), n.double()
    den = n + eps
    out = (T + Y * _coef(Y, T, n, den)[:, None]) / den[:, None]
    if G is not None:
        out = out + abs(a) * G.double().abs()
    if add2 is not None:
        out = out + add2.double().abs()
    return out


def encoder64(A, E0, K, gamma, eps=EPS):
    """gamma E0 + (1 - gamma) mean(X_1 .. X_K), X_k = A rownorm(X_(k-1)); A a float64 matrix (dense or sparse), E0 float64."""
    X, layers = E0, []
    for _ in range(K):
        X = X / (torch.norm(X, dim=1) + eps)[:, None]
        X = torch.sparse.mm(A, X) if A.is_sparse else A @ X
        layers.append(X)
    return gamma * E0 + (1.0 - gamma) * torch.stack(layers, dim=1).mean(dim=1)
