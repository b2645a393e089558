"""The SimGCL / XSimGCL / SGL family on the GPU against its float64 statement (tests/ssl_ref64.py): the Philox noise epilogue of
idg_graph.hip in every instantiation, idg_perturb_f32, idg_propagate_mean_noise_f32, idg_propagate_views_f32 and the `ssl` /
`xssl` / `sgl` branches of the engine's fused step, at epsilon > 0.  The noise is a function of (seed, stream, row, feature
block), so the statement replays on the host exactly the uniforms a kernel drew.

Stream mapping the replay uses (tests/ssl_ref64.py states it in full).  A call naming (seed, s) draws s itself
(idg_perturb_f32, idg_spmm_noise_f32).  A K-layer pass drawn as (seed, sid): idg_propagate_mean_noise_f32 draws sid * 64 + k in
layer k; idg_propagate_views_f32 and ops.propagate_views_raw's composition (shared first product: layer 0 not in the mean,
K >= 2, a tiled width) draw sid * 64 in layer 1 and sid * 64 + (k - 1) in layer k; every other ops.propagate_views_raw call is
idg_propagate_mean_noise_f32 per view.  The engine: seed = torch.cuda.initial_seed(); SimGCL's step i draws sid 2i - 1 and 2i,
XSimGCL's sid i, and its layer-1 view again on sid * 64 + 1.

Tolerances.  (a), (b): elementwise |out - ref| <= 2^-24 |ref| + (d / 2 + 4) 2^-24 eps u_hat — the float32 sum of d squares is
within (d + 1) 2^-24 relative in any order, sqrt halves it, sqrt / division / sign * u add 3 * 2^-24, the final fmaf rounds
once; a wrong uniform, norm or stream word is an error of order eps u_hat itself, 1e5 times the bound.  Entries with sign 0 are
returned bit for bit.  (c)-(g): egcf_ref64.band() — the kernel may sit at max(4 e_f32, 8 * 2^-24) of max |ref64|, e_f32 being
the distance of the SAME statement evaluated in float32; each loss on its own scale.  Tables and moments after three steps:
tests/test_gpu_directau.py's trajectory criterion against adam64 fed the float64 gradients (under 1e-3 of the elements outside
rtol 1e-4 / atol 1e-6, none further than 1e-4).  Nothing is left out of a comparison: every case asserts, with the float64
statement alone, that no layer output has a fragile entry (ssl_ref64.fragile; tests/test_ssl_ref.py asserts the same on the
CPU, where the table seeds, the stream base and the batch offset were searched).

Measured on an MI355X (120 tests, 8 s), as e_kernel against its yardstick e_f32 where a band applies.
(a) at most 0.40 of the derived bound (d = 4).  (b) at most 0.944 of it (d = 32, every handle: entries where u_hat is small and
the final fmaf's rounding, 2^-24 |ref|, is all there is); d = 48 with a bitmap is refused (the restricted kernels exist for the
tiled widths).  (c) closest to its band 1.61e-7 against 1.01e-7 (0.34 of the band); the exact_order handle 8.62e-7 and 5.40e-7
against the reference-order yardstick's 8.13e-7 and 5.14e-7 (the dense float32 product: 2.09e-7 and 1.35e-7).  (d) closest
5.99e-7 against 4.39e-7 (view 1 - view 2, graph_small, K = 3; 0.34), at most 1.35e-6 anywhere.  (e) outputs 1.45e-7 against
1.25e-7 (0.29), gradients 1.23e-7 against 1.50e-7 (0.21).  (f) losses within 8.9e-7 relative, closest XSimGCL's InfoNCE term 1.73e-7
against 4.35e-8 (0.36: under the floor); gradients closest 6.10e-7 against 5.15e-7 (XSimGCL K = 4, 0.30), at most 6.9e-6 where
the float32 statement itself sits at 3.4e-5; after three steps at most 5.7e-5 of a table's elements outside rtol 1e-4 / atol
1e-6 (XSimGCL K = 2; none for the moments), at most 5.8e-6 off, the moments within 4.9e-6 of their largest entry.  (g) closest
2.57e-6 against 2.02e-6 (XSimGCL, B = 5; 0.32); SGL at B = 1: max |g64| 9.8e-3, the cancelling terms' scale 0.75.
The comparison found one defect: a row-restricted product on an exact_order handle also wrote (correct values into) the rows
beyond a tile that were NOT requested — spmm_xl_kernel did not read the bitmap; (b) on that handle fails without the fix.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import ssl_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
EPS = ref.EPS
HANDLES = {"default": {}, "split64": {"split_threshold": 64}, "exact": {"exact_order": True}}
WORST = {}  # group -> [e_kernel, e_f32] of the comparison with the largest e_kernel / band (printed by the last test)


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


@pytest.fixture(scope="module")
def golden_next():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "next_small.npz")))


class _Case:
    """One graph: its CSR, the dense float64 / float32 operators on the device, and its handles (opened on first use)."""

    def __init__(self, ops, name, csr):
        self.ops, self.name = ops, name
        self.indptr, self.indices, self.values, self.n, self.U = csr
        self.A64 = ref.dense_operator(self.indptr, self.indices, self.values, (self.n, self.n), device="cuda")
        self.A32 = self.A64.float()
        self.S32 = ref.sparse_operator(self.indptr, self.indices, self.values, (self.n, self.n))  # (on the CPU: the reference's order)
        self._handles = {}

    def A(self, dtype):
        return self.A64 if dtype == F64 else self.A32

    def handle(self, which="default"):
        if which not in self._handles:
            self._handles[which] = self.ops.Graph(self.indptr, self.indices, self.values, self.n, self.n, **HANDLES[which])
        return self._handles[which]


@pytest.fixture(scope="module")
def graphs(ops, golden_small):
    """graph_small.npz's adjacency, and the 2,500-user / 900-item zipf graph with hub rows (ssl_ref64.hub_graph) — opened three
    ways: default (tile kernels, chunked hubs), split_threshold = 64 (split-row combine) and exact_order (long-row streaming)."""
    out = {"small": _Case(ops, "small", ref.small_graph(golden_small)), "hub": _Case(ops, "hub", ref.hub_graph())}
    hub = out["hub"]
    assert int(np.diff(hub.indptr).max()) > 2048
    assert (np.asarray(hub.handle().long_rows()[2]) > 0).sum() >= 2  # at least two rows are chunked
    info = {k: hub.handle(k).info() for k in HANDLES}
    print("hub handles:", info)
    assert info["split64"]["n_long_rows"] > info["default"]["n_long_rows"]  # rows of 65+ entries are split as well
    assert info["exact"]["flags"] != info["default"]["flags"]
    assert float((hub.A64 - hub.A64.t()).abs().max()) == 0  # symmetric: the backward reuses the handle
    return out


def _bitmap(rows, n):
    return torch.from_numpy(ref.bitmap_of(rows, n)).cuda()


def _rows_of(case):
    """(rows, bitmap) a restricted call asks for: on the hub graph the hub rows, an empty row and 400 others."""
    if case.name == "hub":
        rows, empty = ref.hub_rows()
        assert np.diff(case.indptr)[empty] == 0 and all(case.U + i in rows for i in ref.HUB_ITEMS)
    else:
        rows = np.unique(np.concatenate([np.random.default_rng(8).choice(case.n, 150, replace=False), [0, case.n - 1, case.U + 40]]))
    return torch.from_numpy(rows).cuda(), _bitmap(rows, case.n)


def _note(group, e_k, e_f):
    w = WORST.setdefault(group, [0.0, 0.0, 0.0])
    if e_k / ref.band(e_f) >= w[2]:
        w[:] = [e_k, e_f, e_k / ref.band(e_f)]


def _check(group, what, got, ref64, f32, scale=None):
    """f32: the float32 evaluation of the statement, or several of them (the yardstick is the one furthest from float64)."""
    if isinstance(f32, (list, tuple)):
        e_k, e_f = max(ref.errors(got, ref64, f, scale) for f in f32)
    else:
        e_k, e_f = ref.errors(got, ref64, f32, scale)
    print("  (%s) %-62s e_kernel %.2e  e_f32 %.2e" % (group, what, e_k, e_f))
    _note(group, e_k, e_f)
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


def _check_perturbed(group, what, out, want64, uhat, eps, d, sign, base, sel=None):
    """The derived elementwise bound of (a) / (b); entries with sign 0 equal `base` bit for bit.  Returns the largest
    |out - ref| / bound."""
    if sel is not None:
        out, want64, uhat, sign, base = out[sel], want64[sel], uhat[sel], sign[sel], base[sel]
    assert bool(torch.isfinite(out).all()), what
    err = (out.double() - want64).abs()
    bound = 2.0 ** -24 * want64.abs() + (d / 2 + 4) * 2.0 ** -24 * eps * uhat
    worst = float((err / bound.clamp_min(1e-300))[sign != 0].max())
    print("  (%s) %-62s |out - ref| at most %.3f of the bound" % (group, what, worst))
    w = WORST.setdefault(group, [0.0])
    w[0] = max(w[0], worst)
    assert bool((err <= bound).all()), "%s: %.3f of the bound, %d entries beyond it (largest error %.3e = %.3f eps u_hat)" % (
        what, worst, int((err > bound).sum()), float(err.max()), float((err / (eps * uhat).clamp_min(1e-300)).max()))
    zero = sign == 0
    assert torch.equal(out[zero], base[zero]), what + ": an entry with sign 0 was moved"
    return worst


# =============================================================================================== (a) the generator, through a kernel
STREAMS_A = [(1234, 5), (ref.NOISE_SEED, ref.SIDS[1])]  # the second: high bits set in the seed and in the stream id


def _sign_pattern(n, d):
    r, f = np.arange(n)[:, None], np.arange(d)[None, :]
    s = (r * 7 + f * 3 + (r * f) // 5) % 3 - 1  # +1, -1, 0 in a fixed pattern
    s[11], s[13] = 0, 1
    return s


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("d", [4, 7, 32, 48, 64, 100, 128, 256, 512])
def test_perturbation_draws_the_stated_uniforms(ops, d, with_rows):
    """ops.perturb_raw on X = s * 2^-20, eps = 1: out - X is s * u_hat, u_hat the statement's normalised uniforms — the counter
    and key words, the 24-bit conversion and the row norm over exactly d features, in the tiled and the any-width kernel."""
    n, eps = 300, 1.0
    s = torch.from_numpy(_sign_pattern(n, d)).cuda().double()
    assert all(int((s == v).sum()) > n * d // 5 for v in (-1, 0, 1))
    X = (s * 2.0 ** -20).float()
    rows = np.nonzero((np.arange(n) % 3 != 1) | (np.arange(n) > 290))[0]
    sel = torch.from_numpy(rows).cuda() if with_rows else torch.arange(n, device="cuda")
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[sel] = False
    for seed, sid in STREAMS_A:
        out = torch.full((n, d), float("nan"), device="cuda")
        ops.perturb_raw(X, eps, seed, sid, out=out, rows=_bitmap(rows, n) if with_rows else None)
        uhat = ref.unit_noise(seed, sid, n, d, F64, "cuda")
        np.testing.assert_allclose(uhat.norm(dim=1).cpu().numpy(), 1.0, rtol=1e-12)
        _check_perturbed("a", "d=%d rows=%s stream=(%#x, %#x)" % (d, with_rows, seed, sid), out, X.double() + s * uhat * eps, uhat,
                         eps, d, s, X, sel)
        assert bool(torch.isnan(out[rest]).all()), "a row outside the bitmap was written"


# =============================================================================================== (b) one perturbed product
def _perturbed_product(ops, case, handle, d, restricted, listed=False):
    from idgrec_amd.native import IdgError

    G = case.handle(handle)
    X = ref.table(case.n, d, 100 + d).cuda()
    t = G.spmm_raw(X)  # (pinned bit for bit to the oracle by tests/test_gpu_parity.py)
    rows, bm = _rows_of(case)
    if restricted and d not in ref.TILED:
        # the row-restricted kernels exist for the tiled widths only: any other width with a bitmap is an error, not a quiet
        # product of every row
        with pytest.raises(IdgError, match="row-restricted output needs d in"):
            ops.spmm_noise_raw(G, X, EPS, ref.NOISE_SEED, ref.SIDS[1], out=torch.empty_like(X), out_rows=bm)
        return
    sel = rows if restricted else torch.arange(case.n, device="cuda")
    seed, sid = ref.NOISE_SEED, ref.SIDS[1]
    units = None
    if listed:
        units = G.live_units(bm, int(rows.numel()))
        torch.cuda.synchronize()
        assert int(units[0].item()) >= int(rows.numel())
    try:
        out = torch.full((case.n, d), float("nan"), device="cuda")
        ops.spmm_noise_raw(G, X, EPS, seed, sid, out=out, out_rows=bm if restricted else None)
        torch.cuda.synchronize()
    finally:
        if listed:
            G.forget_live_units(bm)
    uhat = ref.unit_noise(seed, sid, case.n, d, F64, "cuda")
    want = ref.perturb64(t, EPS, seed, sid)
    _check_perturbed("b", "%s %s d=%d restricted=%s listed=%s" % (case.name, handle, d, restricted, listed), out, want, uhat, EPS, d,
                     torch.sign(t), t, sel)
    rest = torch.ones(case.n, dtype=torch.bool, device="cuda")
    rest[sel] = False
    assert bool(torch.isnan(out[rest]).all()), "a row that was not requested was written"
    empty = torch.from_numpy(np.nonzero(np.diff(case.indptr) == 0)[0]).cuda()
    assert empty.numel() > 0 and bool((t[empty] == 0).all())  # rows without entries: sign 0, not moved (checked above)


@pytest.mark.parametrize("restricted", [False, True])
@pytest.mark.parametrize("d", [32, 64, 256, 48])
@pytest.mark.parametrize("handle", list(HANDLES))
def test_one_perturbed_product_in_every_instantiation(ops, graphs, handle, d, restricted):
    _perturbed_product(ops, graphs["hub"], handle, d, restricted)


def test_one_perturbed_product_with_a_live_unit_list(ops, graphs):
    _perturbed_product(ops, graphs["hub"], "default", 64, True, listed=True)


def test_one_perturbed_product_on_the_small_graph(ops, graphs):
    for restricted in (False, True):
        _perturbed_product(ops, graphs["small"], "default", 64, restricted)


# =============================================================================================== (c) K-layer perturbed passes
def _table(case, d):
    return ref.table(case.n, d, ref.table_seed(case.name, d)).cuda()


@pytest.mark.parametrize("graph,K,inc,d", ref.MEAN_NOISE_CASES)
def test_k_layer_perturbed_pass(ops, graphs, graph, K, inc, d):
    case = graphs[graph]
    E0 = _table(case, d)
    seed, sid = ref.NOISE_SEED, ref.SIDS[0]
    trace = []
    want = ref.propagate_noise64(case.A64, E0, K, inc, EPS, seed, sid, 1, F64, trace)
    assert len(trace) == K and ref.fragile_in(trace, case.A64) == 0
    f32 = ref.propagate_noise64(case.A32, E0, K, inc, EPS, seed, sid, 1, F32)
    every = graph == "hub" and d == 64 and K == 3  # the split-row and the streaming handles once per form of the mean
    for handle in (list(HANDLES) if every else ["default"]):
        got = case.handle(handle).propagate_mean_noise_raw(E0, K, inc, EPS, seed, sid)
        yard = f32
        if handle == "exact":
            # an EXACT_ORDER handle adds a row's products in one chain, in the reference's order (2,371 terms on the largest
            # hub row): its yardstick is the reference's own float32 evaluation, torch.sparse.mm on the CPU (ssl_ref64.
            # sparse_operator), which sits 4 to 5 times further from float64 than the blocked dense product does
            yard = [f32, ref.propagate_noise64(case.S32, E0.cpu(), K, inc, EPS, seed, sid, 1, F32)]
        _check("c", "%s %s K=%d layer0=%s d=%d" % (graph, handle, K, inc, d), got, want, yard)


# =============================================================================================== (d) ops.propagate_views_raw
_expected = {}


def _views_expected(case, K, inc, d, n_views):
    """(float64 views, float32 views) for the first n_views streams: evaluated once per (graph, K, layer 0, d) for three."""
    key = (case.name, K, inc, d)
    if key not in _expected:
        E0 = _table(case, d)
        trace = []
        w64 = ref.views64(case.A64, E0, K, inc, EPS, ref.pass_streams(3), F64, trace)
        w32 = ref.views64(case.A32, E0, K, inc, EPS, ref.pass_streams(3), F32)
        _expected[key] = (w64, w32, [ref.fragile(case.A64, xp, x) for xp, x in trace])
    w64, w32, frag = _expected[key]
    assert len(frag) == 3 * K and sum(frag[:K * n_views]) == 0  # (the streams this case draws)
    return w64[:n_views + 1], w32[:n_views + 1]


ONE_CALL = [c for c in ref.VIEWS_CASES if c[4] <= 2 and not c[2]]
VIEW_RUNS = [(c, r, False) for c in ONE_CALL for r in (False, True)] \
    + [(("hub", 3, False, 64, 2), r, True) for r in (False, True)] \
    + [(c, r, False) for c in ref.VIEWS_CASES if c not in ONE_CALL for r in (False, True)]


@pytest.fixture
def compose_views(ops):
    """compose_views(flag) sets ops._compose_views[0] — the list is mutated, never rebound: propagate_views_raw reads the name in
    its own module — and False is put back after the test."""
    def set_flag(composed):
        ops._compose_views[0] = composed
    yield set_flag
    ops._compose_views[0] = False


@pytest.mark.parametrize("case_,restricted,composed", VIEW_RUNS)
def test_views(ops, graphs, compose_views, case_, restricted, composed):
    """The clean pass and the perturbed views of one call: idg_propagate_views_f32 (shared first product, one multi-panel launch
    for the last layer with a bitmap), the same passes composed from the single-purpose entry points, three views (the
    composition) and layer 0 in the mean (no shared product: idg_propagate_mean_noise_f32 per view)."""
    graph, K, inc, d, n_views = case_
    case = graphs[graph]
    assert ref.shares_first_product(K, inc, d) == (not inc)
    compose_views(composed)
    w64, w32 = _views_expected(case, K, inc, d, n_views)
    rows, bm = _rows_of(case)
    sel = rows if restricted else torch.arange(case.n, device="cuda")
    rest = torch.ones(case.n, dtype=torch.bool, device="cuda")
    rest[sel] = False
    outs = [torch.full((case.n, d), float("nan"), device="cuda") for _ in range(n_views + 1)]
    ops.propagate_views_raw(case.handle(), _table(case, d), K, inc, EPS, ref.pass_streams(n_views), outs, out_rows=bm if restricted else None)
    tag = "%s K=%d layer0=%s d=%d views=%d restricted=%s composed=%s" % (graph, K, inc, d, n_views, restricted, composed)
    for i, (got, a, b) in enumerate(zip(outs, w64, w32)):
        _check("d", tag + (" clean" if i == 0 else " view %d" % i), got[sel], a[sel], b[sel])
        if K <= 3:  # (deeper stacks keep their running sum in the output panel: its other rows hold the earlier layers' sum)
            assert bool(torch.isnan(got[rest]).all()), "a row that was not requested was written"
    for i in range(1, n_views):  # two views of one call differ by what their two streams make them differ by
        _check("d", tag + " view %d - view %d" % (i, i + 1), (outs[i] - outs[i + 1])[sel], (w64[i] - w64[i + 1])[sel],
               (w32[i] - w32[i + 1])[sel])
        assert float((w64[i] - w64[i + 1])[sel].abs().max()) > 0.1 * EPS / d ** 0.5


# =============================================================================================== (e) the autograd forms
@pytest.fixture
def autograd_streams(ops):
    """ops.propagate_views under autograd draws (torch.cuda.initial_seed(), next counter value): both set, and put back."""
    state = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(ref.AUTOGRAD_SEED)
    ops.reset_noise_stream(ref.AUTOGRAD_SID0)
    yield
    torch.cuda.set_rng_state(state)
    ops.reset_noise_stream(0)


@pytest.mark.parametrize("graph,K,inc,d,n_views", ref.AUTOGRAD_CASES)
def test_propagate_views_under_autograd(ops, graphs, autograd_streams, graph, K, inc, d, n_views):
    """Outputs and d sum_i <w_i, out_i> / d E0 with random upstream gradients w_i: ONE backward propagation of the summed
    gradients against the float64 autograd through every pass, sign() constant."""
    case = graphs[graph]
    E0 = _table(case, d)
    gen = torch.Generator(device="cuda").manual_seed(d + K)
    ws = [torch.randn((case.n, d), device="cuda", generator=gen) for _ in range(n_views + 1)]
    x = E0.clone().requires_grad_(True)
    outs = ops.propagate_views(case.handle(), x, K, inc, EPS, n_views=n_views)
    sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    res = {}
    for dtype in (F64, F32):
        e = E0.to(dtype).requires_grad_(True)
        trace = []
        views = ref.views64(case.A(dtype), e, K, inc, EPS, ref.autograd_streams(n_views), dtype, trace)
        (g,) = torch.autograd.grad(sum((o * w.to(dtype)).sum() for o, w in zip(views, ws)), e)
        res[dtype] = ([v.detach() for v in views], g)
        if dtype == F64:
            assert len(trace) == K * n_views and ref.fragile_in(trace, case.A64) == 0
    tag = "%s K=%d layer0=%s d=%d views=%d" % (graph, K, inc, d, n_views)
    for i, o in enumerate(outs):
        _check("e", tag + " output %d" % i, o.detach(), res[F64][0][i], res[F32][0][i])
    _check("e", tag + " d / d E0", x.grad, res[F64][1], res[F32][1])


@pytest.mark.parametrize("graph,d", [("hub", 64), ("small", 48)])
def test_spmm_perturbed_under_autograd(ops, graphs, graph, d):
    case = graphs[graph]
    X = _table(case, d)
    stream = (ref.NOISE_SEED, ref.SIDS[2])
    w = torch.randn((case.n, d), device="cuda", generator=torch.Generator(device="cuda").manual_seed(d))
    x = X.clone().requires_grad_(True)
    Y = ops.spmm_perturbed(case.handle(), x, EPS, stream=stream)
    (Y * w).sum().backward()
    res = {}
    for dtype in (F64, F32):
        e = X.to(dtype).requires_grad_(True)
        P = case.A(dtype) @ e
        if dtype == F64:
            assert ref.fragile(case.A64, X, P.detach()) == 0
        y = ref.perturb64(P, EPS, stream[0], stream[1], dtype)
        (g,) = torch.autograd.grad((y * w.to(dtype)).sum(), e)
        res[dtype] = (y.detach(), g)
    _check("e", "spmm_perturbed %s d=%d output" % (graph, d), Y.detach(), res[F64][0], res[F32][0])
    _check("e", "spmm_perturbed %s d=%d d / d X" % (graph, d), x.grad, res[F64][1], res[F32][1])


# =============================================================================================== (f), (g) the fused steps
def _model(name, layers, tmp_path, golden_small, golden_next, graphs, ops):
    """(model, optimizer, configuration, float64 operators, extra arguments of the step) after tools.set_seed(2024) and
    ops.reset_noise_stream(0)."""
    import importlib

    import scipy.sparse as sp

    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    g, nx, case = golden_small, golden_next, graphs["small"]
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", name + ".txt"), name)
    cfg["GCN_layer"] = str(layers)
    assert cfg == ref.read_config(name, GCN_layer=layers)
    d = tmp_path / "small"
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(tmp_path) + "/")
    data = data_loader.Data(str(d), cfg)
    tools.set_seed(2024)
    ops.reset_noise_stream(0)
    assert int(torch.cuda.initial_seed()) == ref.ENGINE_SEED
    m = getattr(importlib.import_module("models." + name), name)(cfg, data, torch.device("cuda")).to("cuda")
    m.keep_fused_grad = True
    assert np.array_equal(m._storage.cpu().numpy(), np.concatenate([g["d64_init_user"], g["d64_init_item"]]))
    eye = torch.eye(case.n, device="cuda")
    assert torch.equal(m.Graph.spmm_raw(eye), case.A32)  # the model's operator is the one the statement multiplies by
    mats, extra = [case.A64], ()
    if name == "SGL":
        subs = [sp.csr_matrix((nx[k + "_data"], nx[k + "_indices"], nx[k + "_indptr"]), shape=(case.n, case.n)) for k in ("sgl_sub1", "sgl_sub2")]
        extra = tuple(tools.convert_sp_mat_to_graph(s, torch.device("cuda")) for s in subs)
        mats += [ref.dense_operator(s.indptr, s.indices, s.data, s.shape, device="cuda") for s in subs]
        for G, M in zip(extra, mats[1:]):
            assert torch.equal(G.spmm_raw(eye), M.float())
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    return m, opt, cfg, mats, extra


def _fused_step(m, opt, name, how, bt, extra, loss):
    if name == "SGL":
        assert m.fused_sgl_step(*bt, *extra, loss, opt)
    elif how == "train_step":
        assert m.fused_train_step(*bt, loss, opt)
    else:  # the gradient panel written out, Adam as its own pass: the engine's other backward
        m.fused_loss_and_grad(*bt, loss)
        opt.step()
    return torch.cat([m.user_embedding.weight.grad, m.item_embedding.weight.grad]).clone()


def _statement(name, mats, W, U, bt, cfg, i, check_fragile=True):
    trace = []
    l64, g64 = ref.engine_step64(name, mats, W, U, bt, cfg, i, F64, trace)
    if name != "SGL":
        assert len(trace) == int(cfg["GCN_layer"]) * (2 if name == "SimGCL" else 1)
    assert not check_fragile or ref.fragile_in(trace, mats[0]) == 0
    l32, g32 = ref.engine_step64(name, [M.float() for M in mats], W, U, bt, cfg, i, F32)
    return l64, g64, l32, g32


def _compare_step(group, tag, loss, grad, l64, g64, l32, g32, ssl_scale=None, grad_scale=None):
    for k, lname in enumerate(("bpr", "reg", "ssl")):
        _check(group, "%s loss %s" % (tag, lname), loss[k], l64[k], l32[k], ssl_scale if k == 2 else None)
    _check(group, tag + " gradient", grad, g64, g32, grad_scale)


@pytest.mark.parametrize("name,layers,how", [(n, k, "train_step") for n, k in ref.FUSED_RUNS]
                         + [("XSimGCL", k, "loss_and_grad") for k in (2, 3, 4)])
def test_fused_steps_against_the_float64_statement(ops, graphs, tmp_path, golden_small, golden_next, name, layers, how):
    """Three fused steps at the shipped epsilon: the three losses and the gradient of every step against the float64 step
    evaluated at the float32 table the step started from, with the streams the engine draws; the table and both moments
    after the third against adam64 fed those float64 gradients.  XSimGCL through fused_train_step is the one-chain Horner form
    (the view's gradient rows ride on the last product, Adam in its epilogue), through fused_loss_and_grad + optimizer.step()
    the other backward."""
    m, opt, cfg, mats, extra = _model(name, layers, tmp_path, golden_small, golden_next, graphs, ops)
    U = graphs["small"].U
    W0 = m._storage.detach().clone()
    grads = []
    loss = torch.zeros((3, 3), device="cuda")
    for i, bt in enumerate(ref.fused_batches(golden_small), 1):
        bt = tuple(x.cuda() for x in bt)
        want = _statement(name, mats, m._storage.detach().clone(), U, bt, cfg, i)
        grad = _fused_step(m, opt, name, how, bt, extra, loss[i - 1])
        _compare_step("f", "%s K=%d %s step %d" % (name, layers, how, i), loss[i - 1], grad, *want)
        grads.append(want[1])
    W, M, V = ref.adam64(W0, grads, lr=float(cfg["learn_rate"]))[-1]
    st_u, st_i = opt.state[m.user_embedding.weight], opt.state[m.item_embedding.weight]
    assert int(st_u["step"]) == 3 and int(st_i["step"]) == 3
    for what, mine, want in (("table", m._storage, W), ("exp_avg", torch.cat([st_u["exp_avg"], st_i["exp_avg"]]), M),
                             ("exp_avg_sq", torch.cat([st_u["exp_avg_sq"], st_i["exp_avg_sq"]]), V)):
        mine, want = mine.detach().cpu().numpy(), want.cpu().numpy()
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        far = float(np.abs(mine - want).max())
        print("  (f) %s K=%d %s %s after three steps: %.2e of the elements outside the band, at most %.2e off (%.2e of the "
              "largest entry)" % (name, layers, how, what, off.mean(), far, far / np.abs(want).max()))
        assert off.mean() < 1e-3, (what, off.mean())
        assert far < 1e-4, (what, far)
    assert float((m._storage - W0).abs().max()) > 1e-3


ISOLATED_ITEM = 40  # an item of graph_small.npz without a training interaction: a zero row of every propagated panel
SMALL_BATCHES = {"repeats": ([3, 3, 7, 9, 3], [1, 5, ISOLATED_ITEM, 6, 1], [100, 2, 8, ISOLATED_ITEM, 30]), "one": ([4], [8], [100])}


@pytest.mark.parametrize("batch", list(SMALL_BATCHES))
@pytest.mark.parametrize("name,how", [("SimGCL", "train_step"), ("XSimGCL", "train_step"), ("XSimGCL", "loss_and_grad"), ("SGL", "train_step")])
def test_small_batches_through_the_engine(ops, graphs, tmp_path, golden_small, golden_next, name, how, batch):
    """B = 5 with one user three times (one of its triples twice) and an isolated item as a positive and as a negative — a zero
    row in every view: sign(0) = 0, the row is not moved — and B = 1, one step each."""
    m, opt, cfg, mats, extra = _model(name, 3, tmp_path, golden_small, golden_next, graphs, ops)
    case = graphs["small"]
    assert np.diff(case.indptr)[case.U + ISOLATED_ITEM] == 0
    bt = tuple(torch.tensor(x, dtype=torch.int64, device="cuda") for x in SMALL_BATCHES[batch])
    W = m._storage.detach().clone()
    want = _statement(name, mats, W, case.U, bt, cfg, 1)
    loss = torch.zeros(3, device="cuda")
    grad = _fused_step(m, opt, name, how, bt, extra, loss)
    # B = 1: each side's InfoNCE is -log(1 + 1e-5) whatever the views hold, so the term is ssl_lambda * -2e-5 and carries the
    # rounding of the log's ARGUMENT (2^-24 of 1, passed on one to one) — 6e-3 of the term itself.  It is compared on the
    # argument's scale, ssl_lambda; every other loss on its own.
    lam, t = float(cfg["ssl_lambda"]), float(cfg["temperature"])
    grad_scale = None
    if batch == "one":
        # ... and its gradient vanishes identically: the occurrence's terms, ssl_lambda * b / (T ||x||) each (x the view's row, b a
        # unit vector), cancel, and what a float32 evaluation leaves of them lives on THEIR scale (tests/test_gpu_egcf.py, the
        # same case of the same kernel).  It reaches E0 where the view contains it — SGL's mean over layers 0 .. K, a quarter
        # of it E0 itself — so there the gradient is compared on max(max |g64|, ssl_lambda / ((K + 1) T min ||x||));
        # SimGCL's and XSimGCL's views reach E0 through A only and are held to max |g64|.
        if name == "SGL":
            rows = torch.stack([bt[0][0], case.U + bt[1][0]])
            x = torch.cat([ref.propagate_clean64(M, W, 3, True)[rows] for M in mats[1:]])
            grad_scale = max(float(want[1].abs().max()), lam / (4 * t * float(x.norm(dim=1).min())))
            print("  (g) SGL B=1: max |g64| %.3e, the cancelling terms' scale %.3e" % (float(want[1].abs().max()), grad_scale))
    _compare_step("g", "%s %s B=%d" % (name, how, len(SMALL_BATCHES[batch][0])), loss, grad, *want,
                  ssl_scale=lam if batch == "one" else None, grad_scale=grad_scale)
    eng = m.engine()
    if batch == "repeats" and name != "SGL":
        assert bool((eng.final[case.U + ISOLATED_ITEM] == 0).all()) and bool((eng._views[0][case.U + ISOLATED_ITEM] == 0).all())
    if batch == "one":
        assert abs(float(want[0][2]) + 2 * lam * np.log1p(10e-6)) < 1e-12 * lam


def test_report_worst_figures():
    """Prints, per group, the comparison that came closest to its bound (what the module docstring quotes)."""
    for group in sorted(WORST):
        w = WORST[group]
        if len(w) == 1:
            print("  (%s) derived bound: at most %.3f of it" % (group, w[0]))
        else:
            print("  (%s) closest to its band: e_kernel %.2e, e_f32 %.2e (%.2f of the band)" % (group, w[0], w[1], w[2]))
