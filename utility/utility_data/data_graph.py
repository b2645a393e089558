"""Normalised adjacency builders with the reference's names, cache files and value bits
(utility/utility_data/data_graph.py:7-79), assembled natively in O(E) instead of through
SciPy DOK/LIL (336 s at yelp2018 scale).

Each function returns a scipy CSR matrix exactly as the reference does (float32 for the plain
graph, float64 for the self-loop graph) and reads/writes the same `.npz` cache files in the
dataset directory, so caches are interchangeable with the reference's.
"""
import numpy as np
import scipy.sparse as sp

from idgrec_amd import host as _host


def _cached(data, name, build):
    path = data.path + "/" + name
    try:
        mat = sp.load_npz(path + ".npz")
        print("\t Adjacency matrix loading completed.")
    except Exception:  # the reference rebuilds on ANY load failure (data_graph.py:37)
        mat = build()
        try:
            sp.save_npz(path, mat)
        except OSError as err:  # read-only dataset directory: keep going without a cache
            print("\t (adjacency cache not written: %s)" % err)
        print("\t Adjacency matrix constructed.")
    return mat


def _bipartite(data, self_loops):
    n = data.num_users + data.num_items
    indptr, indices, values = _host.build_norm_adj(data.num_users, data.num_items, data.train_user, data.train_item,
                                                   self_loops=self_loops)
    mat = sp.csr_matrix((values, indices, indptr), shape=(n, n))
    return mat.astype(np.float64) if self_loops else mat


def sparse_adjacency_matrix(data):
    """D^-1/2 [[0,R],[R^T,0]] D^-1/2 (cache: pre_A.npz)."""
    return _cached(data, "pre_A", lambda: _bipartite(data, False))


def sparse_adjacency_matrix_with_self(data):
    """D^-1/2 ([[0,R],[R^T,0]] + I) D^-1/2 (cache: pre_A_with_self.npz)."""
    return _cached(data, "pre_A_with_self", lambda: _bipartite(data, True))


def sparse_adjacency_matrix_asymmetric(data, alpha, beta):
    """D^-alpha [[0,R],[R^T,0]] D^-beta, float32 (cache: pre_A_{alpha}_{beta}.npz, the floats as Python prints them) — the
    adjacency of LightGCN++ (models/LightGCN_pp.py:42-73).  alpha != beta makes it differ from its transpose.  The
    reference's expressions on CSR operands: float32 degrees raised to -alpha and -beta in float32, infinities (a node
    without an edge under a positive exponent) replaced by 0, and every value the float32 product (d_i^-alpha . a_ij) .
    d_j^-beta, left factor first."""
    alpha, beta = float(alpha), float(beta)

    def build():
        R = data.user_item_net.astype(np.float32).tocsr()
        A = sp.bmat([[None, R], [R.T, None]], format="csr", dtype=np.float32)
        A.sort_indices()
        deg = np.array(A.sum(axis=1))  # float32 [n, 1], as the reference's row sums
        with np.errstate(divide="ignore"):
            left = (deg ** -alpha).flatten()
            right = (deg ** -beta).flatten()
        left[np.isinf(left)] = 0.0
        right[np.isinf(right)] = 0.0
        mat = sp.diags(left).dot(A).dot(sp.diags(right)).tocsr()
        mat.sort_indices()
        return mat

    return _cached(data, "pre_A_%s_%s" % (alpha, beta), build)


def sparse_adjacency_matrix_R(data):
    """Rectangular D_u^-1/2 R D_i^-1/2 (cache: pre_R.npz) — used only by models outside the
    LightGCN hot path (EGCF / CVGA / LightGCL); kept on SciPy with the reference's expression."""

    def build():
        R = data.user_item_net
        with np.errstate(divide="ignore"):
            du = np.power(np.array(R.sum(axis=1)), -0.5).flatten()
            di = np.power(np.array(R.sum(axis=0)), -0.5).flatten()
        du[np.isinf(du)] = 0.0
        di[np.isinf(di)] = 0.0
        return sp.diags(du).dot(R).dot(sp.diags(di)).tocsr()

    return _cached(data, "pre_R", build)
