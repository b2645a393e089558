"""The SimGCL / XSimGCL / SGL family stated once more, in numpy and plain torch and (by default) float64: the Philox noise,
the perturbation X += sign(X) * normalize(u) * eps, the perturbed and clean encoder passes and the three training steps.
tests/test_gpu_ssl.py holds the HIP kernels (idg_graph.hip's noise epilogue, idg_perturb_f32, idg_propagate_views_f32) and the
`ssl` / `xssl` / `sgl` branches of the engine against it; tests/test_ssl_ref.py pins it, without a GPU, to the published
Philox vectors and to the reference's own numbers (tests/golden/next_small.npz).  Nothing of the library is imported here.

The generator (include/idgrec.h on idg_spmm_noise_f32; noise4 in idg_graph.hip).  Features f = 4b .. 4b + 3 of row r draw
the four words of ONE Philox4x32-10 block:

    counter = (r & 0xffffffff, r >> 32, b = f >> 2, stream & 0xffffffff)
    key     = (seed & 0xffffffff, (seed >> 32) ^ (stream >> 32))
    u[r, f] = (word[f & 3] >> 8) * 2^-24                      in [0, 1), a multiple of 2^-24

and the row norm of normalize(u) runs over the row's d features only (of a last, partial block: the first d - 4b words).

Which entry point draws which stream, for a pass drawn as (seed, sid) — 64-bit arithmetic, sid * 64 + j wraps:

    idg_spmm_noise_f32 / idg_perturb_f32 (seed, s)               the stream s itself
    idg_propagate_mean_noise_f32 (propagate_common)              layer k = 1 .. K:  sid * 64 + k       first_substream = 1
    ops.layer_noise_stream((seed, sid), k)                       sid * 64 + k (XSimGCL's layers, one by one)
    idg_propagate_views_f32, and ops.propagate_views_raw's       layer 1: sid * 64  (the shared product A.E0, perturbed per
      composition of the same passes (shared first product)      view); layer k = 2 .. K: sid * 64 + (k - 1)   first_substream = 0
    ops.propagate_views_raw otherwise (layer 0 in the mean,      idg_propagate_mean_noise_f32 per view: sid * 64 + k
      K = 1, or a width without tiled kernels)

The engine (idgrec_amd/engine.py) takes seed = torch.cuda.initial_seed() and counts sid up from ops.reset_noise_stream(0):
SimGCL's step i (1-based) draws sid = 2i - 1 and 2i through ops.propagate_views_raw; XSimGCL's draws sid = i through
idg_propagate_mean_noise_f32 and its layer-1 view once more on ops.layer_noise_stream(stream, 1) = sid * 64 + 1.

Every function takes `dtype`: torch.float64 is the reference, torch.float32 the SAME expressions in the kernels' number
format — the yardstick for how far a correct float32 evaluation may sit from the reference (egcf_ref64.band)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.egcf_ref64 import FLOOR, adam64, band, dense_operator, deterministic, errors, infonce64  # noqa: F401

M32 = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1
TILED = (32, 64, 128, 256, 512)  # widths with tiled kernels: where ops.propagate_views_raw shares the first product


# ------------------------------------------------------------------------------------------------ the generator
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by the Weyl
    constants after each.  ctr: four, key: two arrays (or ints) of 32-bit words, broadcast; returns four uint64 arrays
    holding 32-bit words."""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & M32 for x in ctr)
    k0, k1 = (np.asarray(x, dtype=np.uint64) & M32 for x in key)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & M32, (p0 >> sh) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def uniforms(seed, stream_id, n, d, rows=None):
    """u[n, d] (float64, exact) of rows 0 .. n - 1 — or of the row ids `rows` — for (seed, stream_id): see the docstring."""
    seed, stream_id = int(seed) & M64, int(stream_id) & M64
    r = np.arange(n, dtype=np.uint64) if rows is None else np.asarray(rows).astype(np.uint64)
    nb = (int(d) + 3) // 4
    b = np.arange(nb, dtype=np.uint64)
    ctr = (r[:, None] & M32, r[:, None] >> np.uint64(32), b[None, :], np.uint64(stream_id & 0xFFFFFFFF))
    key = (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) ^ (stream_id >> 32)))
    words = np.stack(np.broadcast_arrays(*philox4x32_10(ctr, key)), axis=-1)  # [n, nb, 4]
    u = (words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u.reshape(len(r), nb * 4)[:, :d]


def substream(sid, j):
    """sid * 64 + j in the kernels' unsigned 64-bit arithmetic."""
    return (int(sid) * 64 + int(j)) & M64


# ------------------------------------------------------------------------------------------------ the perturbation
def unit_noise(seed, stream_id, n, d, dtype=torch.float64, device="cpu"):
    """u_hat = u / max(||u||_2, 1e-12), row by row over the d features, evaluated in `dtype`."""
    u = torch.from_numpy(uniforms(seed, stream_id, n, d)).to(device=device, dtype=dtype)
    return F.normalize(u, dim=-1, eps=1e-12)


def perturb64(X, eps, seed, stream_id, dtype=torch.float64):
    """X + sign(X) * u / max(||u||_2, 1e-12) * eps (models/SimGCL.py, aggregate(perturbed=True)); sign() carries no
    gradient, as under the reference's autograd."""
    X = X.to(dtype)
    n, d = X.shape
    return X + torch.sign(X).detach() * unit_noise(seed, stream_id, n, d, dtype, X.device) * eps


# ------------------------------------------------------------------------------------------------ the encoders
def propagate_clean64(A, E0, K, include0, dtype=torch.float64):
    """mean over the layers of E_k = A E_{k-1}, k = 1 .. K, with E_0 iff include0."""
    A, X = A.to(dtype), E0.to(dtype)
    terms = [X] if include0 else []
    for _ in range(K):
        X = A @ X
        terms.append(X)
    return torch.stack(terms, dim=1).mean(dim=1)


def propagate_noise64(A, E0, K, include0, eps, seed, sid, first_substream, dtype=torch.float64, trace=None, layers=None):
    """The perturbed pass: layer k is X = A @ X followed by the in-place perturbation on stream sid * 64 + first_substream +
    k - 1; the perturbed layer feeds the next one and enters the mean.  first_substream = 1: idg_propagate_mean_noise_f32;
    0: the shared-first-product path of idg_propagate_views_f32 and its composition.  trace (a list) receives (X_prev,
    A @ X_prev) of every layer, for fragile(); layers (a list) the perturbed layers."""
    A, X = A.to(dtype), E0.to(dtype)
    terms = [X] if include0 else []
    for k in range(1, K + 1):
        P = A @ X
        if trace is not None:
            trace.append((X.detach(), P.detach()))
        X = perturb64(P, eps, seed, substream(sid, first_substream + k - 1), dtype)
        terms.append(X)
        if layers is not None:
            layers.append(X)
    return torch.stack(terms, dim=1).mean(dim=1)


def shares_first_product(K, include0, d):
    """ops.propagate_views_raw's own rule for computing A.E0 once."""
    return (not include0) and K >= 2 and d in TILED


def views64(A, E0, K, include0, eps, streams, dtype=torch.float64, trace=None):
    """[clean, view 1, ...] as ops.propagate_views_raw returns them; streams: [(seed, sid), ...]."""
    first = 0 if shares_first_product(K, include0, E0.shape[1]) else 1
    out = [propagate_clean64(A, E0, K, include0, dtype)]
    for seed, sid in streams:
        out.append(propagate_noise64(A, E0, K, include0, eps, seed, sid, first, dtype, trace))
    return out


def sparse_operator(indptr, indices, values, shape, dtype=torch.float32):
    """The same operator as the coalesced sparse tensor the reference hands to torch.sparse.mm (on the CPU), which adds a row's
    products one after the other in CSR order — the order an IDG_GRAPH_EXACT_ORDER handle reproduces.  Its float32
    evaluation is the yardstick for such a handle: one chain of 2,371 terms on hub_graph()'s largest row sits further from
    float64 than the blocked sums of a dense float32 product do."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(indptr))
    idx = torch.from_numpy(np.stack([rows, np.asarray(indices, dtype=np.int64)]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(values).astype(np.float32)).to(dtype), tuple(shape)).coalesce()


def fragile(A, X_prev, X):
    """How many NON-ZERO entries of the layer output X = A @ X_prev (float64) lie below 16 * 2^-24 * (|A| @ |X_prev|): there a
    float32 product may land on the other side of zero and the perturbation then differs by 2 * eps * u_hat.  Exact zeros
    (rows without entries, zero input rows) are zeros in every format and do not count."""
    A, X_prev, X = A.double(), X_prev.double(), X.double()
    bound = 16 * 2.0 ** -24 * (A.abs() @ X_prev.abs())
    return int(((X != 0) & (X.abs() < bound)).sum())


def fragile_in(trace, A):
    return sum(fragile(A, xp, x) for xp, x in trace)


# ------------------------------------------------------------------------------------------------ the steps
def _bpr_reg(final, E, users, pos, neg, U, reg_lambda):
    """losses.get_bpr_loss (the 10e-8 guard inside the log) and reg_lambda * losses.get_reg_loss over the ego rows."""
    ue, pe, ne = final[users], final[U + pos], final[U + neg]
    x = (ue * pe).sum(dim=1) - (ue * ne).sum(dim=1)
    bpr = torch.mean(-torch.log(torch.sigmoid(x) + 10e-8))
    reg = sum(1 / 2 * blk.norm(2).pow(2) / float(blk.shape[0]) for blk in (E[users], E[U + pos], E[U + neg]))
    return bpr, reg_lambda * reg


def _contrast(v1, v2, users, pos, U, t, unique, dtype):
    ui, ii = (torch.unique(users), torch.unique(pos)) if unique else (users, pos)
    return infonce64(v1[ui], v2[ui], t, dtype) + infonce64(v1[U + ii], v2[U + ii], t, dtype)


def _finish(losses, E):
    losses = torch.stack(losses)
    (dE,) = torch.autograd.grad(losses.sum(), E)
    return losses.detach(), dE


def _ids(E, *lists):
    return tuple(torch.as_tensor(x).long().to(E.device) for x in lists)


def simgcl_step64(A, E0, U, users, pos, neg, K, eps, t, ssl_lambda, reg_lambda, streams, dtype=torch.float64, trace=None):
    """SimGCL.forward (models/SimGCL.py; the reference's models/SimGCL.py:62-90) and its backward: ([bpr, reg_lambda * reg,
    ssl_lambda * (InfoNCE_users + InfoNCE_items)], d sum / d E0) in `dtype`.  E0: the [U + I, d] panel, users first;
    streams: [(seed, sid)] * 2 of the two views, drawn as ops.propagate_views_raw draws them; layer 0 not in the mean;
    InfoNCE over the batch's unique users / positives."""
    E = E0.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = _ids(E, users, pos, neg)
    with deterministic():
        clean, v1, v2 = views64(A, E, K, False, eps, streams, dtype, trace)
        bpr, reg = _bpr_reg(clean, E, users, pos, neg, U, reg_lambda)
        return _finish([bpr, reg, ssl_lambda * _contrast(v1, v2, users, pos, U, t, True, dtype)], E)


def xsimgcl_step64(A, E0, U, users, pos, neg, K, cl_layer, eps, t, ssl_lambda, reg_lambda, stream, dtype=torch.float64,
                   trace=None):
    """XSimGCL.forward (models/XSimGCL.py; the reference's models/XSimGCL.py:69-95): ONE perturbed pass (stream = (seed, sid),
    layer k on sid * 64 + k); BPR reads its layer mean, InfoNCE contrasts layer cl_layer's output (E0 itself when no layer
    matches) with that mean over the batch's unique users / positives."""
    E = E0.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = _ids(E, users, pos, neg)
    with deterministic():
        layers = []
        final = propagate_noise64(A, E, K, False, eps, stream[0], stream[1], 1, dtype, trace, layers)
        view = layers[cl_layer - 1] if 1 <= cl_layer <= K else E
        bpr, reg = _bpr_reg(final, E, users, pos, neg, U, reg_lambda)
        return _finish([bpr, reg, ssl_lambda * _contrast(view, final, users, pos, U, t, True, dtype)], E)


def sgl_step64(A, A1, A2, E0, U, users, pos, neg, K, t, ssl_lambda, reg_lambda, dtype=torch.float64):
    """SGL.forward (models/SGL.py; the reference's models/SGL.py:62-101): the LightGCN encoder (layer 0 in the mean) on the
    full graph and on two sub-graphs; InfoNCE between the sub-graph views over the RAW batch ids (duplicates count)."""
    E = E0.detach().to(dtype).clone().requires_grad_(True)
    users, pos, neg = _ids(E, users, pos, neg)
    with deterministic():
        final, v1, v2 = (propagate_clean64(M, E, K, True, dtype) for M in (A, A1, A2))
        bpr, reg = _bpr_reg(final, E, users, pos, neg, U, reg_lambda)
        return _finish([bpr, reg, ssl_lambda * _contrast(v1, v2, users, pos, U, t, False, dtype)], E)


# ------------------------------------------------------------------------------------------------ the cases
def small_graph(g):
    """(indptr, indices, values, n, U) of tests/golden/graph_small.npz's normalised adjacency."""
    U, I = int(g["num_users"]), int(g["num_items"])
    return g["adj_indptr"], g["adj_indices"], g["adj_data"], U + I, U


def hub_graph():
    """2,500 users x 900 items, zipf item popularity, two item hubs (2,000 and 700 users by construction; the zipf head is
    a third): rows chunked by the tile schedule and one beyond 2,048 entries.  The symmetric normalised adjacency
    D^-1/2 [[0, R], [R^T, 0]] D^-1/2 as sorted CSR with float32 values: (indptr, indices, values, n, U)."""
    rng = np.random.default_rng(67)
    U, I = 2500, 900
    eu = np.concatenate([rng.integers(0, U, 30000), rng.choice(U, 2000, replace=False), rng.choice(U, 700, replace=False)])
    ei = np.concatenate([(rng.zipf(1.3, 30000) % I), np.full(2000, 5), np.full(700, 77)])
    eu, ei = np.unique(np.stack([eu, ei]), axis=1)
    n = U + I
    rows = np.concatenate([eu, ei + U]).astype(np.int64)
    cols = np.concatenate([ei + U, eu]).astype(np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    deg = np.bincount(rows, minlength=n).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)
    vals = (dinv[rows] * dinv[cols]).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return indptr, cols.astype(np.int32), vals, n, U


HUB_ITEMS = (5, 77)  # hub_graph(): the constructed hubs, as item ids


def hub_rows(seed=3):
    """The rows a restricted call asks for on hub_graph(): the hub rows, an empty row (asserted by the callers) and 400
    others."""
    indptr, _, _, n, U = hub_graph()
    deg = np.diff(indptr)
    empty = int(np.nonzero(deg == 0)[0][0])
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([rng.choice(n, 400, replace=False), [U + i for i in HUB_ITEMS], [int(np.argmax(deg))],
                                     [empty]])), empty


def bitmap_of(rows, n):
    bm = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(bm, np.asarray(rows) >> 5, (np.uint32(1) << (np.asarray(rows) & 31).astype(np.uint32)))
    return bm.view(np.int32)


def table(n, d, seed):
    """A float32 [n, d] table, N(0, 0.1^2), as a float32 torch tensor."""
    return torch.from_numpy((np.random.default_rng(seed).standard_normal((n, d)) * 0.1).astype(np.float32))


# The (graph, K, include_layer0, d, table seed) cases of the K-layer tests; noise streams: pass_streams().  The table
# seeds are the smallest (from 1) at which fragile() is 0 in every layer of every pass the case runs — searched on the CPU
# (tests/test_ssl_ref.py re-checks each) — so no comparison leaves an entry out.
EPS = 0.1
NOISE_SEED = (0x5EED << 32) | 1234  # high bits set: the key's second word is seed_hi ^ stream_hi
SIDS = (5, (3 << 32) | 6, 9)  # the second has high bits set as well


def pass_streams(n_views):
    return [(NOISE_SEED, s) for s in SIDS[:n_views]]


TABLE_SEEDS = {("small", 64): 1, ("small", 48): 1, ("small", 256): 1, ("hub", 64): 2, ("hub", 48): 1, ("hub", 256): 53}


def table_seed(graph, d):
    return TABLE_SEEDS[(graph, d)]


# (c) idg_propagate_mean_noise_f32: (graph, K, include_layer0, d)
MEAN_NOISE_CASES = [(gr, K, inc, 64) for gr in ("small", "hub") for K in (1, 2, 3, 4) for inc in (True, False)] \
    + [(gr, 3, False, d) for gr in ("small", "hub") for d in (48, 256)]
# (d) ops.propagate_views_raw: (graph, K, include_layer0, d, n_views)
VIEWS_CASES = [(gr, K, False, 64, nv) for gr in ("small", "hub") for K in (2, 3, 4) for nv in (1, 2)] \
    + [(gr, 3, False, 256, 2) for gr in ("small", "hub")] + [("hub", 3, False, 64, 3), ("hub", 3, True, 64, 2)]
# (e) the autograd forms: ops.propagate_views draws (torch.cuda.initial_seed(), counter + 1 ...) — the tests set both
AUTOGRAD_SEED, AUTOGRAD_SID0 = 2024, 300


def autograd_streams(n_views):
    """What ops.propagate_views draws after torch.cuda.manual_seed(AUTOGRAD_SEED) and ops.reset_noise_stream(AUTOGRAD_SID0)."""
    return [(AUTOGRAD_SEED, AUTOGRAD_SID0 + 1 + v) for v in range(n_views)]


AUTOGRAD_CASES = [("hub", 3, False, 64, 2), ("small", 3, False, 48, 2), ("small", 2, True, 64, 1)]  # (graph, K, include0, d, views)


# ------------------------------------------------------------------------------------------------ the fused runs
ENGINE_SEED = 2024  # tools.set_seed(2024): torch.cuda.initial_seed()
# (model, GCN_layer): configure/<model>.txt with XSimGCL's GCN_layer overridden
# three batches of 256 of graph_small.npz's `sample1`, from this row on: the first offset (in steps of 256) after 0 at which no
# step of any run below has a fragile entry (at 0, step 3 of two runs has one each: tests/test_ssl_ref.py re-checks)
FUSED_BATCH0, FUSED_B = 256, 256
FUSED_RUNS = [("SimGCL", 3), ("XSimGCL", 2), ("XSimGCL", 3), ("XSimGCL", 4), ("SGL", 3)]


def fused_batches(g):
    """[(users, pos, neg)] * 3 (int64 tensors) out of graph_small.npz."""
    tri = torch.from_numpy(g["sample1"][FUSED_BATCH0:FUSED_BATCH0 + 3 * FUSED_B])
    return [tuple(tri[i * FUSED_B:(i + 1) * FUSED_B, c].contiguous() for c in range(3)) for i in range(3)]


def read_config(name, **override):
    """configure/<name>.txt as floats / ints where they parse."""
    import os

    out = {}
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configure", name + ".txt")) as fh:
        for line in fh:
            parts = [x.strip() for x in line.split("=")]
            if len(parts) == 2:
                out[parts[0]] = parts[1]
    out.update({k: str(v) for k, v in override.items()})
    return out


def engine_step64(name, mats, E0, U, batch, cfg, i, dtype=torch.float64, trace=None, seed=ENGINE_SEED):
    """Step i (1-based, counted from ops.reset_noise_stream(0)) of a fused run of model `name` at the table E0, with the
    noise streams the engine draws (module docstring).  mats: [A] or, for SGL, [A, A_sub1, A_sub2]; batch: (users, pos,
    neg); cfg: the model's configuration.  Returns (losses [3], d sum / d E0)."""
    K, t, lam, reg = int(cfg["GCN_layer"]), float(cfg["temperature"]), float(cfg["ssl_lambda"]), float(cfg["reg_lambda"])
    if name == "SimGCL":
        return simgcl_step64(mats[0], E0, U, *batch, K, float(cfg["epsilon"]), t, lam, reg, [(seed, 2 * i - 1), (seed, 2 * i)],
                             dtype, trace)
    if name == "XSimGCL":
        return xsimgcl_step64(mats[0], E0, U, *batch, K, int(cfg["cl_layer"]), float(cfg["epsilon"]), t, lam, reg, (seed, i),
                              dtype, trace)
    assert name == "SGL"
    return sgl_step64(mats[0], mats[1], mats[2], E0, U, *batch, K, t, lam, reg, dtype)
