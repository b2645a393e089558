"""The nnz partitioner and shard extraction of the user-row-sharded step (see step.py for the algorithm)."""
import numpy as np


# --------------------------------------------------------------------------- partitioning
def partition_users_by_nnz(user_degree, world):
    """Contiguous user blocks with ~equal stored entries.  Returns bounds[world + 1]."""
    deg = np.asarray(user_degree, dtype=np.int64)
    U = len(deg)
    csum = np.concatenate([[0], np.cumsum(deg)])
    total = csum[-1]
    bounds = [0]
    for r in range(1, world):
        target = total * r // world
        b = int(np.searchsorted(csum, target, side="left"))
        bounds.append(min(max(b, bounds[-1]), U))
    bounds.append(U)
    return np.asarray(bounds, dtype=np.int64)


def shard_adjacency(indptr, indices, values, num_users, num_items, u_lo, u_hi):
    """From the global normalised adjacency CSR ([U+I, U+I], users first) cut
    R_g   (rows = users [u_lo, u_hi), columns = items 0..I)  and
    R_g^T (rows = items 0..I, columns = users re-based to 0..u_hi-u_lo).
    Values are copied, never re-normalised."""
    U, I = int(num_users), int(num_items)
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices)
    values = np.asarray(values, dtype=np.float32)
    # user rows: every column is an item (>= U)
    s, e = indptr[u_lo], indptr[u_hi]
    ui_ptr = indptr[u_lo:u_hi + 1] - s
    ui_idx = (indices[s:e].astype(np.int64) - U).astype(np.int32)
    ui_val = values[s:e].copy()
    # item rows: keep the columns that fall in this rank's user block
    s2, e2 = indptr[U], indptr[U + I]
    cols = indices[s2:e2].astype(np.int64)
    keep = (cols >= u_lo) & (cols < u_hi)
    row_of = np.repeat(np.arange(I, dtype=np.int64), np.diff(indptr[U:U + I + 1]))
    iu_cnt = np.bincount(row_of[keep], minlength=I)
    iu_ptr = np.concatenate([[0], np.cumsum(iu_cnt)]).astype(np.int64)
    iu_idx = (cols[keep] - u_lo).astype(np.int32)
    iu_val = values[s2:e2][keep].copy()
    return (ui_ptr, ui_idx, ui_val), (iu_ptr, iu_idx, iu_val)


def shard_adjacency_from_edges(users, items, num_users, num_items, u_lo, u_hi):
    """The same two pieces as shard_adjacency, straight from the interaction list — sorted by (user, item), no
    duplicate pairs (what synth.generate returns) — without building the global [U+I, U+I] CSR first: at configs[4]
    size that build is 4e8 entries and ~55 s per rank, of which a rank keeps 1/N.  Values are the reference's float32
    arithmetic (data_graph.py:46-51: np.power(rowsum, -0.5) in float32, (D.A).D left to right), i.e. bit for bit what
    host.build_norm_adj + shard_adjacency give (tests/test_sharded.py)."""
    U, I = int(num_users), int(num_items)
    users = np.asarray(users, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    if len(users) > 1:
        du = np.diff(users)
        if (du < 0).any() or ((du == 0) & (np.diff(items) <= 0)).any():
            raise ValueError("shard_adjacency_from_edges needs edges sorted by (user, item) without duplicates")
    deg = np.concatenate([np.bincount(users, minlength=U), np.bincount(items, minlength=I)]).astype(np.float32)
    with np.errstate(divide="ignore"):
        dinv = np.power(deg, np.float32(-0.5))
    dinv[np.isinf(dinv)] = 0.0
    s, e = np.searchsorted(users, [u_lo, u_hi], side="left")
    su, si = users[s:e], items[s:e]
    ui_ptr = np.concatenate([[0], np.cumsum(np.bincount(su - u_lo, minlength=u_hi - u_lo))]).astype(np.int64)
    ui_idx = si.astype(np.int32)
    ui_val = (dinv[su] * np.float32(1.0)) * dinv[U + si]
    order = np.argsort(si, kind="stable")  # item rows, users ascending inside each
    iu_ptr = np.concatenate([[0], np.cumsum(np.bincount(si, minlength=I))]).astype(np.int64)
    iu_idx = (su[order] - u_lo).astype(np.int32)
    iu_val = (dinv[U + si[order]] * np.float32(1.0)) * dinv[su[order]]
    return (ui_ptr, ui_idx, ui_val.astype(np.float32)), (iu_ptr, iu_idx, iu_val.astype(np.float32))
