"""csrc/idg_kmeans.hip: k-means (NCL's E-step)."""
import torch

from ..native import check, lib
from ._base import _cached_ws, _ptr, _require_device, _stream


KMEANS_MAX_WIDTH = 256
_kmeans_ws_cache = {}


def _kmeans_ws_bytes(N, K, d):
    nbytes = int(lib.idg_kmeans_workspace_bytes(int(N), int(K), int(d)))
    if nbytes == 0:
        raise ValueError("kmeans_workspace: sizes that are not built (N=%d, K=%d, d=%d)" % (N, K, d))
    return nbytes


def kmeans_workspace(N, K, d, device):
    """A private idg_kmeans_* buffer: the padded copies of X and C, the per-chunk minima and the sorted row ids
    (O((N + K) d + chunks N)), never N x K."""
    return torch.empty(_kmeans_ws_bytes(N, K, d), dtype=torch.uint8, device=device)


def _kmeans_args(who, X, K, C=None, assign=None, ws=None, **outs):
    """The checks of the k-means calls; returns (N, d, ldx, ws).  X: [N, d] float32 with unit column stride (a row stride above
    d — a column slice of a wider panel — is passed through as ldx)."""
    if X.dim() != 2:
        raise ValueError("%s: X must be [N, d]" % who)
    N, d = (int(v) for v in X.shape)
    K = int(K)
    if N < 1 or K < 1:
        raise ValueError("%s: bad sizes (N = %d, K = %d)" % (who, N, K))
    if d < 1 or d > KMEANS_MAX_WIDTH:
        raise ValueError("%s: width %d (1 .. %d is built)" % (who, d, KMEANS_MAX_WIDTH))
    if X.dtype != torch.float32 or X.stride(1) != 1 or (N > 1 and X.stride(0) < d):
        raise TypeError("%s: X must be float32 with contiguous rows (got %s, strides %s)" % (who, X.dtype, tuple(X.stride())))
    if C is not None and (C.dtype != torch.float32 or not C.is_contiguous() or tuple(C.shape) != (K, d)):
        raise TypeError("%s: the centroids must be a contiguous float32 [%d, %d] tensor" % (who, K, d))
    if assign is not None and (assign.dtype != torch.int32 or not assign.is_contiguous() or tuple(assign.shape) != (N,)):
        raise TypeError("%s: assign must be a contiguous int32 [%d] tensor" % (who, N))
    for name, (t, dtype, shape) in outs.items():
        if t is not None and (t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape):
            raise TypeError("%s: %s must be a contiguous %s tensor of shape %s" % (who, name, dtype, shape))
    _require_device(X, C, assign, ws, *[t for t, _, _ in outs.values()])
    if ws is None:
        ws = _cached_ws(_kmeans_ws_cache, (N, K, d, X.device), lambda: _kmeans_ws_bytes(N, K, d), X.device)
    return N, d, (int(X.stride(0)) if N > 1 else d), ws


def kmeans_assign_raw(X, C, assign=None, dist2=None, ws=None):
    """idg_kmeans_assign_f32: assign[i] = argmin_j ||X[i] - C[j]||^2 (int32, ties to the lowest j) and, when `dist2` is given,
    that squared distance.  Returns assign."""
    K = C.shape[0] if C.dim() == 2 else 0
    if assign is None and X.dim() == 2:
        assign = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    N, d, ldx, ws = _kmeans_args("kmeans_assign_raw", X, K, C, assign, ws,
                                 dist2=(dist2, torch.float32, (int(X.shape[0]),) if X.dim() == 2 else ()))
    check(lib.idg_kmeans_assign_f32(_ptr(X), ldx, N, d, _ptr(C), int(K), _ptr(assign), _ptr(dist2), _ptr(ws), _stream()),
          "idg_kmeans_assign_f32")
    return assign


def kmeans_update_raw(X, assign, C, counts=None, ws=None):
    """idg_kmeans_update_f32: C[j] <- the mean of the rows of X with assign[i] = j, in place (a cluster without rows keeps its
    centroid); counts (optional int32 [K]) <- the rows per cluster.  Returns C."""
    K = C.shape[0] if C.dim() == 2 else 0
    N, d, ldx, ws = _kmeans_args("kmeans_update_raw", X, K, C, assign, ws, counts=(counts, torch.int32, (int(K),)))
    check(lib.idg_kmeans_update_f32(_ptr(X), ldx, N, d, _ptr(assign), int(K), _ptr(C), _ptr(counts), _ptr(ws), _stream()),
          "idg_kmeans_update_f32")
    return C


def kmeans_raw(X, C, niter, assign=None, inertia=None, ws=None):
    """idg_kmeans_f32: niter x (assign, update) from the centroids in C (updated in place), then the assignment against the
    final centroids; inertia (optional float32 [niter + 1]) <- the sum of squared distances of every assignment.  One chain
    of launches, nothing read back.  Returns (C, assign)."""
    niter = int(niter)
    if niter < 0:
        raise ValueError("kmeans_raw: niter = %d" % niter)
    K = C.shape[0] if C.dim() == 2 else 0
    if assign is None and X.dim() == 2:
        assign = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    N, d, ldx, ws = _kmeans_args("kmeans_raw", X, K, C, assign, ws, inertia=(inertia, torch.float32, (niter + 1,)))
    check(lib.idg_kmeans_f32(_ptr(X), ldx, N, d, int(K), niter, _ptr(C), _ptr(assign), _ptr(inertia), _ptr(ws), _stream()),
          "idg_kmeans_f32")
    return C, assign


def kmeans(X, K, niter=25, seed=1234):
    """Lloyd's k-means of the rows of X [N, d] on the device (what models/NCL.py:66-74 asks of faiss.Kmeans + index.search):
    (centroids [K, d], assign int32 [N], inertia [niter + 1]).  The initial centroids are the rows
    torch.randperm(N, generator=<CPU generator seeded with `seed`>)[:K] of X: distinct rows, the same row indices for the same
    N and seed.  A cluster that loses all its rows keeps its centroid."""
    if X.dim() != 2:
        raise ValueError("kmeans: X must be [N, d]")
    N, K = int(X.shape[0]), int(K)
    if K < 1 or K > N:
        raise ValueError("kmeans: K = %d clusters for N = %d rows" % (K, N))
    if X.dtype != torch.float32:
        raise TypeError("kmeans: X must be float32 (got %s)" % X.dtype)
    _require_device(X)
    first = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:K].to(X.device)
    C = X.detach().index_select(0, first).contiguous()
    inertia = torch.empty(int(niter) + 1, dtype=torch.float32, device=X.device)
    C, assign = kmeans_raw(X.detach(), C, niter, inertia=inertia)
    return C, assign, inertia
