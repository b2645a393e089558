"""The length-balanced second tile schedule of the dense SpMM launches (idg_graph.hip, idg_tile_packer.h): every
product, epilogue and fused training step gives the SAME BITS on a handle that carries it as on one that does not
(ops.Graph(balanced_tiles=False)), and the restricted / sparse-input / unit-list forms and masked copies — which stay
on the first schedule — are untouched by its presence.

Graphs: a symmetric bipartite adjacency whose user degrees hit every case of the work decomposition (0, 1, 7, 8, 9, 63,
64, 65, 128, 129, 300, 512, 513 and ~1100 entries: whole rows, rows split in LDS, one- and three-chunk rows with a short
last chunk) beside several hundred short rows, and a non-bipartite square matrix large enough for the 8-band placement."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WIDTHS = [32, 64, 128, 256]
FORCED = [0, 1, 7, 8, 9, 63, 64, 65, 128, 129, 300, 512, 513, 1100]
U, I = 420, 1200


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bitmap(rows, n):
    w = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(w, np.asarray(rows) >> 5, np.uint32(1) << (np.asarray(rows) & 31).astype(np.uint32))
    return dev(w.view(np.int32))


@pytest.fixture(scope="module")
def bipartite():
    """(indptr, indices, values) of the normalised adjacency, n = U + I, and the interaction lists."""
    import idgrec_amd.host as H

    rng = np.random.default_rng(7)
    deg = np.concatenate([FORCED, rng.integers(1, 13, U - len(FORCED))])
    users = np.repeat(np.arange(U), deg).astype(np.int64)
    items = np.concatenate([np.sort(rng.choice(I, int(k), replace=False)) for k in deg]).astype(np.int64)
    ip, ix, dv = H.build_norm_adj(U, I, users, items)
    assert set(FORCED) <= set(np.diff(ip)[:U].tolist())
    return ip, ix, dv, users, items


@pytest.fixture(scope="module")
def square():
    """A non-symmetric square matrix: ~100 tiles of the first schedule (8 bands), a few hub rows."""
    rng = np.random.default_rng(11)
    n = 6000
    deg = rng.poisson(8, n)
    deg[[5, 2000, 5999]] = [700, 1500, 260]
    deg[rng.integers(0, n, 200)] = 0
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = np.concatenate([np.sort(rng.choice(n, int(k), replace=False)) for k in deg]).astype(np.int32)
    values = rng.standard_normal(len(indices)).astype(np.float32)
    return indptr, indices, values, n


@pytest.fixture(scope="module")
def panels():
    """One gathered panel per width (6000 rows: the first 1620 serve the bipartite graph), drawn once."""
    rng = np.random.default_rng(3)
    return {d: rng.standard_normal((6000, d)).astype(np.float32) for d in WIDTHS}


def _pair(ops, csr, n, **kw):
    on = ops.Graph(csr[0], csr[1], csr[2], n, n, **kw)
    off = ops.Graph(csr[0], csr[1], csr[2], n, n, balanced_tiles=False, **kw)
    si, so = on.schedule_info(), off.schedule_info()
    assert si["balanced"]["tiles"] > 0 and so["balanced"]["tiles"] == 0, (si, so)
    assert si["balanced"]["rounds"] == si["base"]["rounds"] == so["base"]["rounds"]  # the same work
    assert si["balanced"]["utilisation"] > si["base"]["utilisation"], si
    return on, off


def _graphs(ops, which, bipartite, square):
    if which == "bipartite":
        return _pair(ops, bipartite, U + I) + (U + I,)
    return _pair(ops, square, square[3], symmetric=False, build_transpose=False) + (square[3],)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("which", ["bipartite", "square"])
def test_every_dense_epilogue_gives_the_same_bits(which, d, fused, bipartite, square, panels, monkeypatch):
    import idgrec_amd.native as native
    import idgrec_amd.ops as ops

    monkeypatch.setenv("IDG_FUSED_FIX", fused)  # in-kernel last-arriver combine / separate fix-up launch
    on, off, n = _graphs(ops, which, bipartite, square)
    assert on.info()["n_segments"] > 0  # chunked rows: the global partial slots and arrival counters are in play
    X = dev(panels[d][:n])
    rng = np.random.default_rng(d)
    A = dev(rng.standard_normal((n, d)).astype(np.float32))
    S = dev(rng.standard_normal((n, d)).astype(np.float32))
    live = bitmap(rng.choice(n, n // 3, replace=False), n)

    def both(fn):
        a, b = fn(on), fn(off)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        return a

    # plain, twice on one handle: the second launch finds the arrival counters at zero again
    y = both(lambda g: (g.spmm_raw(X), g.spmm_raw(X)))
    assert torch.equal(y[0], y[1])

    def addend_mask(g):
        Y = torch.zeros((n, d), device="cuda")
        ops.spmm_epi_raw(g, X, Y=Y, addend=A, mask=live)
        return (Y,)

    def sum_div(g):
        Y, O = torch.zeros((n, d), device="cuda"), torch.zeros((n, d), device="cuda")
        ops.spmm_ex_raw(g, X, Y=Y, sum_in=S, sum_out=O, div=3.0)
        return Y, O

    def accumulate(g):
        O = A.clone()
        ops.spmm_ex_raw(g, X, sum_out=O, accumulate=True)
        return (O,)

    def noise(g):
        return (ops.spmm_noise_raw(g, X, 0.1, 1234, 5),)

    def act(g):
        Y = torch.zeros((n, d), device="cuda")
        ops.spmm_epi_raw(g, X, Y=Y, act=native.ACT_TANH)
        return (Y,)

    def adam(g):
        p, m, v, G = A.clone(), S.clone() * 0.01, S.clone().abs() * 0.01, torch.zeros((n, d), device="cuda")
        ops.spmm_epi_raw(g, X, sum_out=G, adam=(p, m, v, 1e-3, 3))
        return p, m, v, G

    for fn in (addend_mask, sum_div, accumulate, noise, act):
        both(fn)
    p, m, v, G = both(adam)
    # ... and against the product followed by the stand-alone Adam kernel
    p2, m2, v2, G2 = A.clone(), S.clone() * 0.01, S.clone().abs() * 0.01, torch.zeros((n, d), device="cuda")
    ops.spmm_ex_raw(off, X, sum_out=G2)
    ops.adam_step_raw(p2, G2, m2, v2, 1e-3, 3)
    torch.cuda.synchronize()
    assert torch.equal(G, G2) and torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)


def test_product_against_float64(bipartite, square, panels):
    import idgrec_amd.ops as ops
    import scipy.sparse as sp

    for which in ("bipartite", "square"):
        on, _, n = _graphs(ops, which, bipartite, square)
        ip, ix, dv = (bipartite if which == "bipartite" else square)[:3]
        X = panels[64][:n]
        A = sp.csr_matrix((dv.astype(np.float64), ix, ip), shape=(n, n))
        ref = A @ X.astype(np.float64)
        scale = abs(A) @ np.abs(X.astype(np.float64))
        Y = on.spmm_raw(dev(X)).cpu().numpy()
        # the bound of the existing SpMM tests (test_gpu_parity.py): |err| <= c eps sum |a x|
        assert (np.abs(Y - ref) <= 2e-6 * scale + 1e-30).all()


def test_restricted_forms_and_masked_copy_are_untouched(bipartite, panels):
    import idgrec_amd.ops as ops

    n, d = U + I, 64
    on, off = _pair(ops, bipartite, n)
    X = dev(panels[d][:n])
    rng = np.random.default_rng(21)
    rows = np.unique(np.concatenate([np.arange(len(FORCED)), rng.choice(n, 200, replace=False)]))  # every forced row
    out_rows, x_rows = bitmap(rows, n), bitmap(rng.choice(n, 300, replace=False), n)
    Xs = X.clone()
    dead = np.setdiff1d(np.arange(n), np.flatnonzero(np.unpackbits(x_rows.cpu().numpy().view(np.uint8), bitorder="little")[:n]))
    Xs[dev(dead)] = 0  # x_rows promises that the other rows of the panel are zero

    def forms(g):
        res = []
        Y = torch.zeros((n, d), device="cuda")
        ops.spmm_ex_raw(g, X, Y=Y, out_rows=out_rows)  # restricted: visits the tiles of the first schedule
        res.append(Y)
        Y = torch.zeros((n, d), device="cuda")
        ops.spmm_ex_raw(g, Xs, Y=Y, x_rows=x_rows)  # sparse input
        res.append(Y)
        ws = g.live_units(out_rows, len(rows))  # unit list
        Y = torch.zeros((n, d), device="cuda")
        ops.spmm_ex_raw(g, X, Y=Y, out_rows=out_rows)
        res.append(Y)
        g.forget_live_units(out_rows)
        del ws
        c = g.dropout_copy(0.7, stream=(99, 1))  # masked copy: borrows the first schedule only
        assert c.schedule_info()["balanced"]["tiles"] == 0
        res.append(c.spmm_raw(X))
        res.append(c.T.spmm_raw(X))
        torch.cuda.synchronize()
        return res

    a, b = forms(on), forms(off)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    full = on.spmm_raw(X)
    assert torch.equal(a[0][dev(rows)], full[dev(rows)]) and torch.equal(a[0], a[2])
    assert torch.equal(a[1], on.spmm_raw(Xs))


@pytest.mark.parametrize("K,lookahead", [(3, True), (2, False)])
def test_ten_fused_steps_give_the_same_bits(K, lookahead, bipartite):
    import idgrec_amd.ops as ops
    from idgrec_amd.engine import PropagationEngine

    ip, ix, dv, users, items = bipartite
    n, d, B, steps = U + I, 64, 96, 10
    rng = np.random.default_rng(5)
    W0 = dev((rng.standard_normal((n, d)) * 0.1).astype(np.float32))
    pick = rng.integers(0, len(users), steps * B)
    cols = [dev(users[pick]), dev(items[pick]), dev(rng.integers(0, I, steps * B).astype(np.int64))]
    res = []
    for g in _pair(ops, bipartite, n):
        eng = PropagationEngine(g, U, I, d, K, include_layer0=True, reg_lambda=1e-4, lr=1e-3, params=W0.clone())
        losses = torch.zeros((steps, 2), device="cuda")
        batch = lambda i: tuple(c[i * B:(i + 1) * B] for c in cols)  # noqa: E731
        for i in range(steps):
            if lookahead and i + 1 < steps:
                eng.prefetch(*batch(i + 1))
            eng.train_step(*batch(i), loss_out=losses[i])
        torch.cuda.synchronize()
        assert eng._plan is not None  # the fused one-call step ran
        res.append((eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), losses.clone()))
    for x, y in zip(*res):
        assert torch.isfinite(x).all() and torch.equal(x, y)
