"""EGCF's fused kernels against float64, across their dispatch (reference statement: tests/egcf_ref64.py, pinned to the
reference's own numbers by tests/test_egcf_ref.py):

  (a) the in-batch InfoNCE in EGCF's two forms — the cross form and the shared-panel raw-list pair form — at every shape
      where idg_ssl.hip takes another kernel or loop, with id lists that repeat 2, 5, 70 and B times;
  (b) the tanh / tanh' epilogues of idg_spmm_epi_f32 with every option the engines combine them with;
  (c) idg_rows_tanh_bwd_f32 and idg_lincomb_f32;
  (d) EgcfEngine / EgcfAltEngine for K = 1..4, two steps each, losses, gradient and Adam state.

One tolerance rule throughout (egcf_ref64.errors / band): with scale = max |ref64|,
    e_kernel = max |kernel - ref64| / scale   <=   max(4 e_f32, 8 * 2^-24),   e_f32 = max |float32 composition - ref64| / scale
where the float32 composition is the same plain-torch expressions in float32, run in the same test.  Both numbers are
printed (pytest -s).  Where a case has NO scale of its own — a gradient that is exactly zero by symmetry (one row; every
position the same pair) — the accumulate target's prefill supplies it, sized by the terms that cancel: see _infonce_case."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import egcf_ref64 as ref  # noqa: E402

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _bitmap(n, rows):
    """int32 [ceil(n / 32)] device bitmap with the bits of `rows` set."""
    rows = np.asarray(rows, dtype=np.int64)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return dev(words.view(np.int32))


def _check(what, got, ref64, f32, scale=None):
    e_k, e_f = ref.errors(got, ref64, f32, scale)
    print("  %-58s e_kernel %.2e  e_f32 %.2e" % (what, e_k, e_f))
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


# =============================================================================================== (a) in-batch InfoNCE
def _id_lists(pattern, B, U, I, rng):
    if pattern == "random":
        return rng.integers(0, U, B), rng.integers(0, I, B)
    if pattern == "same":
        return np.full(B, int(rng.integers(0, U))), np.full(B, int(rng.integers(0, I)))
    if pattern == "twice":  # every id exactly twice (an odd B leaves one single), the two lists shuffled on their own
        half = (B + 1) // 2
        users = rng.permutation(np.tile(rng.choice(U, half, replace=False), 2)[:B])
        items = rng.permutation(np.tile(rng.choice(I, half, replace=False), 2)[:B])
        return users, items
    users, items = rng.choice(U, B, replace=False), rng.choice(I, B, replace=False)
    if pattern == "hub":  # one item on 70 positions (past the 64-wide scan and the 4-at-a-time loop), one user on 5
        p = rng.choice(B, 70, replace=False)
        items[p] = items[p[0]]
        q = rng.choice(B, 5, replace=False)
        users[q] = users[q[0]]
    else:
        assert pattern == "distinct"
    return users, items


def _infonce_case(ops, form, d, B, pattern, t, zero_row=False):
    """One call of the cross or the shared-panel pair form with g prefilled, against prefill + 0.1 * (float64 autograd of
    infonce64 on the gathered rows).  The prefill is uniform in +-(gradient scale): 0.1 max |dref|, or — where the gradient
    vanishes identically (B = 1; every position the same pair: b_i - sum_k Q_ik b_k = 0) — 0.1 / (t min ||x||), the size
    of the B occurrences' terms w_i b_i / ||x|| that cancel (sum_i |w_i| ~ 1 / t): the scale their rounding lives on."""
    rng = np.random.default_rng(_seed(form, d, B, pattern, t, zero_row))
    # the issue's 700 + 500 row panel; lists that need more than 500 distinct ids get the 3000 + 5000 one
    U, I = (700, 500) if (B <= 500 or pattern == "random") else (3000, 5000)
    n = U + I
    users, items = _id_lists(pattern, B, U, I, rng)
    panel = (rng.standard_normal((n, d)) * 0.5 + 0.3).astype(np.float32)
    zr = None
    if zero_row:
        zr = int(users[7])
        assert (users == zr).sum() == 1
        panel[zr] = 0.0
    v, users, items = dev(panel), dev(users.astype(np.int64)), dev(items.astype(np.int64))

    def composed(dtype):
        vv = v.to(dtype).clone().requires_grad_(True)
        with ref.deterministic():  # (the gathers' backward adds an id's occurrences: in a fixed order)
            if form == "cross":
                terms = [ref.infonce64(vv[users], vv[U + items], t, dtype)]
            else:
                terms = [ref.infonce64(vv[users], vv[users], t, dtype), ref.infonce64(vv[U + items], vv[U + items], t, dtype)]
            (g,) = torch.autograd.grad(sum(terms), vv)
        return torch.stack(terms).detach(), g

    l64, g64 = composed(F64)
    l32, g32 = composed(F32)
    touched = torch.zeros(n, dtype=torch.bool, device="cuda")
    touched[users] = True
    touched[U + items] = True
    general = touched.clone()
    if zr is not None:
        general[zr] = False
    if pattern == "same" or B == 1:
        gscale = 0.1 / (t * float(v[touched].double().norm(dim=1).min()))
    else:
        gscale = 0.1 * float(g64[general].abs().max())
    prefill = dev((rng.uniform(-1.0, 1.0, (n, d)) * gscale).astype(np.float32))
    want64 = prefill.double() + 0.1 * g64
    want32 = prefill + 0.1 * g32
    ws = ops.infonce_workspace(n, B, d, "cuda")
    outs = []
    for _ in range(2):
        g, loss = prefill.clone(), torch.zeros(2, device="cuda")
        if form == "cross":
            ops.infonce_cross_raw(v, users, items, U, t, g=g, loss=loss, grad_scale=0.1, ws=ws)
        else:
            ops.infonce_pair_raw(v, v, users, items, U, t, g1=g, g2=g, loss=loss, dedup=False, accumulate=True, grad_scale=0.1,
                                 ws=ws)
        outs.append((loss[:len(l64)].clone(), g))
    loss, g = outs[0]
    tag = "%s d=%d B=%d %s t=%.1f" % (form, d, B, pattern, t)
    for k in range(len(l64)):
        _check("%s loss[%d]" % (tag, k), loss[k], l64[k], l32[k])
    _check(tag + " grad", g[general], want64[general], want32[general])
    if zr is not None:  # the clamped row's gradient is of order 1 / 1e-12: on its own scale
        _check(tag + " grad of the zero row", g[zr], want64[zr], want32[zr])
        assert float(want64[zr].abs().max()) > 1e6 * gscale
    assert torch.equal(g[~touched], prefill[~touched]), "a row named by neither id list was written"
    assert torch.equal(outs[1][0], loss) and torch.equal(outs[1][1], g), "the second call gave other bits"
    return l64


# (d, B): what idg_ssl.hip's infonce_impl dispatches on — matrix cores iff d % 64 == 0 and B % 4 == 0, else SIMT;
# ssl_logits_mfma_kernel<2> iff ceil(B / 128)^2 * sets >= 512, else <1>
SMALL = [(20, 1, "random"),      # one row: loss -log(1 + 1e-5), SIMT
         (64, 4, "distinct"),    # smallest matrix-core call
         (64, 1030, "random"),   # d fits, B % 4 != 0: SIMT fallback, 17 ragged 64-tiles
         ] + [(d, B, p) for (d, B) in ((100, 77),     # SIMT, second ragged lane pass over d
                                       (192, 260))    # <1>, three 64-deep chunks, ragged 128- and 64-tiles
              for p in ("distinct", "hub", "twice", "same")]
LARGE = ["distinct", "hub", "twice"]


@pytest.mark.parametrize("t", [0.1, 0.2])
@pytest.mark.parametrize("d,B,pattern", SMALL)
@pytest.mark.parametrize("form", ["cross", "pair"])
def test_infonce_egcf_forms_vs_float64(ops, form, d, B, pattern, t):
    l64 = _infonce_case(ops, form, d, B, pattern, t)
    if B == 1:
        np.testing.assert_allclose(l64.cpu().numpy(), -np.log(1.0 + 1e-5), rtol=1e-9)


@pytest.mark.parametrize("t", [0.1, 0.2])
@pytest.mark.parametrize("pattern", LARGE)
def test_infonce_pair_form_on_128_row_tiles_vs_float64(ops, pattern, t):
    """B = 1924: ceil(1924 / 128)^2 * 2 sets = 512, the first batch at which the shared-panel form runs
    ssl_logits_mfma_kernel<2>, with a ragged last tile (1924 = 15 * 128 + 4)."""
    _infonce_case(ops, "pair", 64, 1924, pattern, t)


@pytest.mark.parametrize("t", [0.1, 0.2])
@pytest.mark.parametrize("pattern", LARGE)
def test_infonce_cross_form_on_128_row_tiles_vs_float64(ops, pattern, t):
    """B = 2820: 23^2 >= 512, so the cross form's single set runs ssl_logits_mfma_kernel<2>; 2820 = 22 * 128 + 4."""
    _infonce_case(ops, "cross", 64, 2820, pattern, t)


@pytest.mark.parametrize("form", ["cross", "pair"])
def test_infonce_gradient_of_a_zero_row(ops, form):
    """An all-zero panel row among the batch's users: normalize() divides by its eps, the Jacobian is 1 / eps with no
    projection (ssl_contrib_kernel's clamped branch) — loss AND gradient."""
    _infonce_case(ops, form, 64, 96, "distinct", 0.2, zero_row=True)


def test_infonce_dedup_unique_count_below_the_grid(ops):
    """De-duplicated sets with distinct g1 / g2 at B = 2048 on 3000 + 5000 rows: every launch is shaped by B, the unique
    counts (about half of it) are read on the device — blocks and lanes beyond them must leave."""
    U, I, d, B, t = 3000, 5000, 64, 2048, 0.2
    rng = np.random.default_rng(_seed("dedup"))
    v1 = dev((rng.standard_normal((U + I, d)) * 0.5 + 0.3).astype(np.float32))
    v2 = dev((rng.standard_normal((U + I, d)) * 0.5 + 0.3).astype(np.float32))
    users, items = dev(rng.integers(0, U, B)), dev((rng.random(B) ** 3 * I).astype(np.int64))
    ui, ii = torch.unique(users), torch.unique(items)
    assert len(ui) < B - 128 and len(ii) < B - 128

    def composed(dtype):
        a, b = v1.to(dtype).clone().requires_grad_(True), v2.to(dtype).clone().requires_grad_(True)
        terms = [ref.infonce64(a[ui], b[ui], t, dtype), ref.infonce64(a[U + ii], b[U + ii], t, dtype)]
        ga, gb = torch.autograd.grad(sum(terms), (a, b))
        return torch.stack(terms).detach(), ga, gb

    l64, a64, b64 = composed(F64)
    l32, a32, b32 = composed(F32)
    outs = []
    for _ in range(2):
        g1, g2, loss = torch.zeros_like(v1), torch.zeros_like(v2), torch.zeros(2, device="cuda")
        ops.infonce_pair_raw(v1, v2, users, items, U, t, g1=g1, g2=g2, loss=loss, dedup=True,
                             ws=ops.infonce_workspace(U + I, B, d, "cuda"))
        outs.append((loss, g1, g2))
    loss, g1, g2 = outs[0]
    for k in range(2):
        _check("dedup loss[%d]" % k, loss[k], l64[k], l32[k])
    _check("dedup grad view 1", g1, a64, a32)
    _check("dedup grad view 2", g2, b64, b32)
    for g, want in ((g1, a64), (g2, b64)):
        assert (g[want == 0] == 0).all()
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))


# =============================================================================================== operators for (b), (d)
N_USERS, N_ITEMS = 300, 200


def _pattern(cover):
    """300 x 200, ~4 % dense; row 17 and column 23 empty; row 5 (150 entries) and column 9 (160 entries) long enough for
    the handle's row split, which starts at 128 entries, on R and on R^T.  cover: every row and column gets an entry."""
    rng = np.random.default_rng(11)
    M = rng.random((N_USERS, N_ITEMS)) < 0.04
    M[5, rng.choice(N_ITEMS, 150, replace=False)] = True
    M[rng.choice(N_USERS, 160, replace=False), 9] = True
    M[17, :] = False
    M[:, 23] = False
    if cover:
        for r in np.flatnonzero(~M.any(axis=1)):
            M[r, (7 * r + 40) % N_ITEMS] = True
        for c in np.flatnonzero(~M.any(axis=0)):
            M[(11 * c + 60) % N_USERS, c] = True
    return M


class _Operators:
    """R as a rectangular handle (with its transposed handle) and A = [[0, R], [R^T, 0]] as the symmetric one, plus the
    dense float64 matrices of the float32 values the handles were given."""

    def __init__(self, ops, values):
        import scipy.sparse as sp

        M = _pattern(cover=values == "normalised")
        if values == "normalised":  # D_u^-1/2 R D_i^-1/2 (data_graph.sparse_adjacency_matrix_R)
            vals = (1.0 / np.sqrt(np.outer(M.sum(axis=1), M.sum(axis=0))))[M]
        else:
            vals = np.random.default_rng(12).standard_normal(int(M.sum())) * 0.3
        R = sp.csr_matrix((vals.astype(np.float32), np.nonzero(M)), shape=M.shape)
        R.sort_indices()
        A = sp.bmat([[None, R], [R.T, None]], format="csr").astype(np.float32)
        A.sort_indices()
        n = N_USERS + N_ITEMS
        self.R = ops.Graph(R.indptr, R.indices, R.data, N_USERS, N_ITEMS, symmetric=False)
        self.A = ops.Graph(A.indptr, A.indices, A.data, n, n)
        self.R64 = ref.dense_operator(R.indptr, R.indices, R.data, M.shape, device="cuda")
        self.A64 = ref.dense_operator(A.indptr, A.indices, A.data, (n, n), device="cuda")
        assert (self.R64.t() - self.A64[N_USERS:, :N_USERS]).abs().max() == 0


_operators = {}


def _ops_for(ops, values):
    if values not in _operators:
        _operators[values] = _Operators(ops, values)
    return _operators[values]


@pytest.fixture(scope="module")
def rect(ops):
    return _ops_for(ops, "random")


# =============================================================================================== (b) activation epilogues
def _side(rect, side):
    """(handle, dense float64 operator) of R or R^T."""
    return (rect.R, rect.R64) if side == "R" else (rect.R.T, rect.R64.t().contiguous())


def _randn(rng, shape, scale=1.0):
    return dev((rng.standard_normal(shape) * scale).astype(np.float32))


def _nan(rows, d):
    return torch.full((rows, d), float("nan"), device="cuda")


SIDES_WIDTHS = [(s, d) for s in ("R", "RT") for d in (64, 128, 48)]  # 64 / 128: tiled float4 epilogue; 48: generic_epilogue
SIDES_TILED = [(s, d) for s in ("R", "RT") for d in (64, 128)]


@pytest.mark.parametrize("side,d", SIDES_WIDTHS)
def test_spmm_tanh_epilogue(ops, rect, side, d):
    from idgrec_amd import native

    G, D = _side(rect, side)
    rows, cols = D.shape
    rng = np.random.default_rng(_seed("tanh", side, d))
    X = _randn(rng, (cols, d))
    Y = _nan(rows, d)
    ops.spmm_epi_raw(G, X, Y=Y, act=native.ACT_TANH)
    _check("tanh %s d=%d Y" % (side, d), Y, torch.tanh(D @ X.double()), torch.tanh(D.float() @ X))
    assert (Y[17 if side == "R" else 23] == 0).all()  # the empty row: tanh(0)
    # with the layer sum of the last product: sum_out = ((s1 + s2) + s3) + Y
    s = [_randn(rng, (rows, d)) for _ in range(3)]
    Y, S = _nan(rows, d), _nan(rows, d)
    ops.spmm_epi_raw(G, X, Y=Y, sum_in=s[0], sum_in2=s[1], sum_in3=s[2], sum_out=S, act=native.ACT_TANH)
    y64, y32 = torch.tanh(D @ X.double()), torch.tanh(D.float() @ X)
    _check("tanh+sums %s d=%d Y" % (side, d), Y, y64, y32)
    _check("tanh+sums %s d=%d sum_out" % (side, d), S, ((s[0].double() + s[1].double()) + s[2].double()) + y64,
           ((s[0] + s[1]) + s[2]) + y32)


@pytest.mark.parametrize("side,d", SIDES_TILED)
def test_spmm_tanh_epilogue_at_out_rows(ops, rect, side, d):
    from idgrec_amd import native

    G, D = _side(rect, side)
    rows, cols = D.shape
    rng = np.random.default_rng(_seed("tanh-out", side, d))
    X, s1 = _randn(rng, (cols, d)), _randn(rng, (rows, d))
    want = np.unique(np.concatenate([rng.choice(rows, rows // 3, replace=False), [0, 5, 9, 17, 23, rows - 1]]))
    Y, S = _nan(rows, d), _nan(rows, d)
    ops.spmm_epi_raw(G, X, Y=Y, sum_in=s1, sum_out=S, act=native.ACT_TANH, out_rows=_bitmap(rows, want))
    sel = dev(want)
    y64, y32 = torch.tanh(D @ X.double()), torch.tanh(D.float() @ X)
    _check("tanh out_rows %s d=%d Y" % (side, d), Y[sel], y64[sel], y32[sel])
    _check("tanh out_rows %s d=%d sum_out" % (side, d), S[sel], (s1.double() + y64)[sel], (s1 + y32)[sel])
    rest = torch.ones(rows, dtype=torch.bool, device="cuda")
    rest[sel] = False
    assert torch.isnan(Y[rest]).all() and torch.isnan(S[rest]).all(), "a row outside out_rows was written"


@pytest.mark.parametrize("x_rows", [False, True])
@pytest.mark.parametrize("side,d", SIDES_WIDTHS)
def test_spmm_tanh_bwd_epilogue(ops, rect, side, d, x_rows):
    """Y = (A . X + addend at the mask's rows) * (1 - act_src^2); addend rows outside the mask and (x_rows) X rows outside
    x_rows hold NaN: they must not be read.  x_rows names exactly the non-zero rows of X."""
    from idgrec_amd import native

    G, D = _side(rect, side)
    rows, cols = D.shape
    rng = np.random.default_rng(_seed("tanh-bwd", side, d, x_rows))
    X = _randn(rng, (cols, d))
    Xk = X
    xb = None
    if x_rows:
        live = np.unique(np.concatenate([rng.choice(cols, cols // 4, replace=False), [0, 5, 9, cols - 1]]))
        keep = torch.zeros(cols, dtype=torch.bool, device="cuda")
        keep[dev(live)] = True
        Xk = torch.where(keep[:, None], X, torch.full_like(X, float("nan")))
        X = torch.where(keep[:, None], X, torch.zeros_like(X))
        xb = _bitmap(cols, live)
    src = torch.tanh(_randn(rng, (rows, d)))
    masked = np.unique(np.concatenate([rng.choice(rows, rows * 2 // 5, replace=False), [5, 9, 17, 23, rows - 1]]))
    m = torch.zeros(rows, dtype=torch.bool, device="cuda")
    m[dev(masked)] = True
    add = torch.where(m[:, None], _randn(rng, (rows, d)), torch.zeros(1, device="cuda"))
    addk = torch.where(m[:, None], add, torch.full_like(add, float("nan")))
    Y = _nan(rows, d)
    ops.spmm_epi_raw(G, Xk, Y=Y, addend=addk, mask=_bitmap(rows, masked), act=native.ACT_TANH_BWD, act_src=src, x_rows=xb)
    _check("tanh' %s d=%d x_rows=%d" % (side, d, x_rows), Y, (D @ X.double() + add.double()) * (1 - src.double() ** 2),
           (D.float() @ X + add) * (1 - src * src))


@pytest.mark.parametrize("x_rows", [False, True])
@pytest.mark.parametrize("d", [64, 128, 48])
def test_spmm_tanh_bwd_epilogue_below_act_rows(ops, rect, d, x_rows):
    """The symmetric [n, n] operator with act_rows = U (EgcfEngine's last square product): rows below U get the derivative,
    rows from U on are the plain product plus addend."""
    from idgrec_amd import native

    U, n = N_USERS, N_USERS + N_ITEMS
    rng = np.random.default_rng(_seed("act-rows", d, x_rows))
    X = _randn(rng, (n, d))
    Xk, xb = X, None
    if x_rows:
        live = np.unique(np.concatenate([rng.choice(n, n // 4, replace=False), [0, U - 1, U, n - 1]]))
        keep = torch.zeros(n, dtype=torch.bool, device="cuda")
        keep[dev(live)] = True
        Xk = torch.where(keep[:, None], X, torch.full_like(X, float("nan")))
        X = torch.where(keep[:, None], X, torch.zeros_like(X))
        xb = _bitmap(n, live)
    src, add = torch.tanh(_randn(rng, (n, d))), _randn(rng, (n, d))
    src[U:] = float("nan")  # (not read there)
    Y = _nan(n, d)
    ops.spmm_epi_raw(rect.A, Xk, Y=Y, addend=add, act=native.ACT_TANH_BWD, act_src=src, act_rows=U, x_rows=xb)
    p64, p32 = rect.A64 @ X.double() + add.double(), rect.A64.float() @ X + add
    _check("tanh' act_rows d=%d x_rows=%d rows < U" % (d, x_rows), Y[:U], p64[:U] * (1 - src[:U].double() ** 2),
           p32[:U] * (1 - src[:U] * src[:U]))
    _check("tanh' act_rows d=%d x_rows=%d rows >= U" % (d, x_rows), Y[U:], p64[U:], p32[U:])
    # the boundary rows on their own scale: U - 1 is the last row the derivative applies to, U the first it does not
    _check("tanh' act_rows d=%d row U - 1" % d, Y[U - 1], p64[U - 1] * (1 - src[U - 1].double() ** 2),
           p32[U - 1] * (1 - src[U - 1] * src[U - 1]))
    _check("tanh' act_rows d=%d row U" % d, Y[U], p64[U], p32[U])


def test_spmm_activation_refuses_the_adam_epilogue(ops, rect):
    from idgrec_amd import native

    I, U, d = N_ITEMS, N_USERS, 64
    X, out = torch.zeros(U, d, device="cuda"), torch.zeros(I, d, device="cuda")
    p, m, v = (torch.zeros(I, d, device="cuda") for _ in range(3))
    with pytest.raises(native.IdgError):
        ops.spmm_epi_raw(rect.R.T, X, sum_out=out, adam=(p, m, v, 1e-3, 1), act=native.ACT_TANH)
    assert (p == 0).all() and (out == 0).all()


# =============================================================================================== (c) the two small kernels
@pytest.mark.parametrize("rows", ["all", "sparse", "last-word"])
@pytest.mark.parametrize("n,d", [(1, 4), (37, 20), (500, 64)])
def test_rows_tanh_bwd_vs_float64(ops, n, d, rows):
    """out = g * (1 - y^2) at the bitmap's rows, elementwise within 2 * 2^-23 |g| of float64: one rounding of y^2 and one
    of 1 - y^2 (absolute 2^-25 each, or one of 2^-24 when fused), one of the product (2^-24 |g|)."""
    rng = np.random.default_rng(_seed("rtb", n, d, rows))
    g, y = _randn(rng, (n, d)), torch.tanh(_randn(rng, (n, d), 1.5))
    if rows == "all":
        live, bm = np.arange(n), None
    else:
        live = np.unique(rng.choice(n, max(1, n // 10), replace=False)) if rows == "sparse" else \
            np.unique(np.concatenate([rng.choice(n, max(1, n // 10)), np.arange(n - (n % 32 or 32), n)]))
        bm = _bitmap(n, live)
    out = _nan(n, d)
    ops.rows_tanh_bwd_raw(g, y, bm, out)
    sel = dev(live)
    want = g.double() * (1 - y.double() ** 2)
    err = (out[sel].double() - want[sel]).abs()
    assert (err <= 2 * 2.0 ** -23 * g[sel].double().abs()).all(), float((err / g[sel].double().abs()).max())
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[sel] = False
    assert torch.isnan(out[rest]).all(), "a row outside the bitmap was written"


@pytest.mark.parametrize("count", [1, 3, 4, 7, 64 * 200 + 2])
def test_lincomb_vs_float64(ops, count):
    rng = np.random.default_rng(count)
    x, y = _randn(rng, (count,)), _randn(rng, (count,))
    a, b = float(np.float32(0.37)), float(np.float32(-1.25))
    out = torch.full((count,), float("nan"), device="cuda")
    ops.lincomb_raw(out, x, a)
    assert torch.equal(out, a * x)
    out = torch.full((count,), float("nan"), device="cuda")
    ops.lincomb_raw(out, x, a, y, b)
    ax, by = a * x.double(), b * y.double()
    assert ((out.double() - (ax + by)).abs() <= 2.0 ** -23 * (ax.abs() + by.abs())).all()


# =============================================================================================== (d) the engines
ENGINE_CASES = [("parallel", 64, 1, 256), ("parallel", 64, 2, 256), ("parallel", 128, 4, 1024), ("parallel", 32, 3, 97),
                ("alternating", 64, 1, 256), ("alternating", 128, 2, 1024), ("alternating", 32, 4, 97),
                ("alternating", 64, 3, 256)]
REG, SSL, TAU, LR = 1e-4, 0.1, 0.1, 1e-3
_engine_runs = {}


def _batch(rng, B, third):
    """B triples from one third of the users and of the items; one positive item on 70 positions, one user on 5."""
    u0, i0 = third * (N_USERS // 3), third * (N_ITEMS // 3)
    users = u0 + rng.integers(0, N_USERS // 3, B)
    pos = i0 + rng.integers(0, N_ITEMS // 3, B)
    neg = i0 + rng.integers(0, N_ITEMS // 3, B)
    p = rng.choice(B, 70, replace=False)
    pos[p] = pos[p[0]]
    q = rng.choice(B, 5, replace=False)
    users[q] = users[q[0]]
    return tuple(dev(x.astype(np.int64)) for x in (users, pos, neg))


def _engine_run(ops, mode, d, K, B):
    """Two training steps of the case's engine with store_grad, every step next to egcf_step64 in float64 and float32 FROM
    THE ENGINE'S OWN TABLE read back before the step; then the same two steps without store_grad."""
    key = (mode, d, K, B)
    if key in _engine_runs:
        return _engine_runs[key]
    from idgrec_amd.egcf import EgcfAltEngine, EgcfEngine

    g = _ops_for(ops, "normalised")
    rng = np.random.default_rng(_seed("engine", *key))
    bound = np.sqrt(6.0 / (N_ITEMS + d))  # nn.init.xavier_uniform_ on [I, d]
    W0 = dev(rng.uniform(-bound, bound, (N_ITEMS, d)).astype(np.float32))
    batches = [_batch(rng, B, 0), _batch(rng, B, 1)]

    def make(store_grad):
        if mode == "parallel":
            return EgcfEngine(g.A, g.R, N_USERS, N_ITEMS, d, K, W0, REG, SSL, TAU, lr=LR, store_grad=store_grad)
        return EgcfAltEngine(g.R, N_USERS, N_ITEMS, d, K, W0, REG, SSL, TAU, lr=LR, store_grad=store_grad)

    eng = make(True)
    steps = []
    for users, pos, neg in batches:
        before = eng.item_table().clone()
        loss = eng.train_step(users, pos, neg).clone()
        st = dict(loss=loss, grad=eng.grad_items().clone(), table=eng.item_table().clone(), M=eng.M.clone(), V=eng.V.clone())
        for name, dtype in (("64", F64), ("32", F32)):
            st["loss" + name], st["grad" + name] = ref.egcf_step64(g.R64, g.A64, before, users, pos, neg, K, mode, REG, SSL, TAU,
                                                                   dtype=dtype)
        steps.append(st)
    assert eng.step_count == 2
    lean = make(False)
    for users, pos, neg in batches:
        lean.train_step(users, pos, neg)
    assert lean.grad_items() is None
    run = dict(W0=W0, steps=steps, lean=(lean.item_table().clone(), lean.M.clone(), lean.V.clone()))
    torch.cuda.synchronize()
    _engine_runs[key] = run
    return run


@pytest.mark.parametrize("mode,d,K,B", ENGINE_CASES)
def test_engine_two_steps_vs_float64(ops, mode, d, K, B):
    run = _engine_run(ops, mode, d, K, B)
    names = ("bpr", "reg", "ssl")
    for s, st in enumerate(run["steps"], 1):
        tag = "%s d=%d K=%d B=%d step %d" % (mode, d, K, B, s)
        for k in range(3):
            _check("%s loss %s" % (tag, names[k]), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " dE", st["grad"], st["grad64"], st["grad32"])


@pytest.mark.parametrize("mode,d,K,B", ENGINE_CASES)
def test_engine_adam_state_after_each_step(ops, mode, d, K, B):
    """exp_avg, exp_avg_sq and the table after each of the two steps against the float64 recurrence fed the engine's own
    two gradients from the float32 initial table: the moments within 4 * 2^-24 of their largest entry, the table within
    4 ulp of its largest entry (bias corrections of step 1 and step 2; rows outside a batch still move by their moments)."""
    run = _engine_run(ops, mode, d, K, B)
    want = ref.adam64(run["W0"], [st["grad"] for st in run["steps"]], lr=LR)
    for s, (st, (W, M, V)) in enumerate(zip(run["steps"], want), 1):
        for name, got, w in (("exp_avg", st["M"], M), ("exp_avg_sq", st["V"], V)):
            e = float((got.double() - w).abs().max() / w.abs().max())
            print("  %s d=%d K=%d step %d %s: %.2f * 2^-24 of max" % (mode, d, K, s, name, e * 2.0 ** 24))
            assert e <= 4 * 2.0 ** -24, (name, s, e)
        wmax = float(W.abs().max())
        ulp = float(np.spacing(np.float32(wmax)))
        e = float((st["table"].double() - W).abs().max())
        print("  %s d=%d K=%d step %d table: %.2f ulp of max |W| = %.3f" % (mode, d, K, s, e / ulp, wmax))
        assert e <= 4 * ulp, (s, e / ulp)
    assert not torch.equal(run["steps"][0]["table"], run["steps"][1]["table"])


@pytest.mark.parametrize("mode,d,K,B", ENGINE_CASES)
def test_engine_without_stored_gradient_is_bit_identical(ops, mode, d, K, B):
    run = _engine_run(ops, mode, d, K, B)
    last = run["steps"][-1]
    for got, want in zip(run["lean"], (last["table"], last["M"], last["V"])):
        assert torch.equal(got, want)


def test_one_layer_engines_agree(ops):
    """K = 1: the two encoders are one function of the table (A's rows are R's and R^T's), so EgcfEngine — which skips the
    middle backward loop and hands x_rows = bitmap to its last square product — and EgcfAltEngine must agree with each
    other within the band, on both steps.  (The table the parallel engine holds before a step is copied into the other:
    a gradient entry of rounding size may flip sign between the two and move its weight by a whole Adam step.)"""
    from idgrec_amd.egcf import EgcfAltEngine, EgcfEngine

    g = _ops_for(ops, "normalised")
    d, B = 64, 256
    rng = np.random.default_rng(_seed("k1"))
    bound = np.sqrt(6.0 / (N_ITEMS + d))
    W0 = dev(rng.uniform(-bound, bound, (N_ITEMS, d)).astype(np.float32))
    par = EgcfEngine(g.A, g.R, N_USERS, N_ITEMS, d, 1, W0, REG, SSL, TAU, lr=LR, store_grad=True)
    alt = EgcfAltEngine(g.R, N_USERS, N_ITEMS, d, 1, W0, REG, SSL, TAU, lr=LR, store_grad=True)
    for s, (users, pos, neg) in enumerate([_batch(rng, B, 0), _batch(rng, B, 1)], 1):
        before = par.item_table().clone()
        alt.item_table().copy_(before)
        lp, la = par.train_step(users, pos, neg).clone(), alt.train_step(users, pos, neg).clone()
        l64, g64 = ref.egcf_step64(g.R64, g.A64, before, users, pos, neg, 1, "parallel", REG, SSL, TAU)
        l32, g32 = ref.egcf_step64(g.R64, g.A64, before, users, pos, neg, 1, "alternating", REG, SSL, TAU, dtype=F32)
        for k, name in enumerate(("bpr", "reg", "ssl")):
            e_f = ref.errors(lp[k], l64[k], l32[k])[1]
            e = abs(float(lp[k]) - float(la[k])) / abs(float(l64[k]))
            print("  K=1 step %d loss %s: |parallel - alternating| %.2e  e_f32 %.2e" % (s, name, e, e_f))
            assert e <= ref.band(e_f)
        e_f = ref.errors(par.grad_items(), g64, g32)[1]
        e = float((par.grad_items().double() - alt.grad_items().double()).abs().max() / g64.abs().max())
        print("  K=1 step %d dE: |parallel - alternating| %.2e  e_f32 %.2e" % (s, e, e_f))
        assert e <= ref.band(e_f)
