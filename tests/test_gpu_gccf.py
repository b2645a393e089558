"""LR-GCCF's layer kernels (idgrec_amd/csrc/idg_gccf.hip), their differentiable wrapper (ops.gccf_layer), the fused step
(idgrec_amd/gccf.py) and the plugin (models/GCCF.py) on the device.  The reference statement is tests/gccf_ref64.py, pinned to
the reference's own numbers by tests/test_gccf_host.py.

  (a) the message-dropout mask of the forward kernel, bit for bit against ngcf_ref64.keep_mask, and untouched memory;
  (b) idg_gccf_layer_fwd_f32 / idg_gccf_layer_bwd_f32 against float64: 1, 2, 3 and more than 512 blocks, gE / gN / both,
      no bitmap / a 5 % bitmap / first and last row only, E written into and gN read from a slot of a wider panel, NaN in
      unread memory, fully dropped rows;
  (c) run to run: two calls give equal bits, the parameter gradients included;
  (d) ops.gccf_layer under autograd: the raw calls' bits at d = 64, the composition of existing operators at d = 128;
  (e) GccfEngine, two consecutive steps with different batches: losses, every gradient, Adam state, parameters;
  (f) models.GCCF against the reference's goldens (tests/golden/gccf_small.npz): losses, gradients, rating, trajectory.

One tolerance rule throughout (b), (d), (e) (egcf_ref64.errors / band): with scale = max |ref64| of the tensor compared,
    e_kernel = max |kernel - ref64| / scale   <=   max(4 e_f32, 8 * 2^-24),   e_f32 = max |float32 composition - ref64| / scale
where the float32 composition is gccf_ref64's same expressions in float32, run in the same test; both numbers are printed
(pytest -s).  The layer is linear between mask and product: no kink case exists to exempt.  Kernel and reference share the
graph's float32 values (dense_operator), the mask and its float32 scale (keep_mask) and the float32 rounding of reg_lambda.
The Adam state of (e) follows tests/test_gpu_ngcf.py::test_engine_adam_state_after_each_step: the float64 recurrence fed the
engine's own gradients, moments within 4 * 2^-24 of their largest entry, parameters within 4 ulp of theirs.  (f) uses the
tolerances of tests/test_gpu_models.py::test_ngcf_vs_reference (losses, gradients, rating) and of
tests/test_gpu_lgcnpp.py::test_model_matches_reference_goldens (the three-step trajectory).

Measured on an MI355X (42 tests, 5.1 .. 5.4 s for the whole file once the library is loaded), e_kernel / e_f32 over all
comparisons of a group, worst e_kernel / band:
  (a) exact: every E equals keep_mask bit for bit, every other bit of the panels is the NaN it was (5 tests, 60 panels)
  (b) 0 .. 4.7e-7 / 0 .. 3.4e-6 (0.49: n = 65, p = 0, gE + gN at rows 0 and n - 1, gb), 378 comparisons
  (d) 1.3e-7 .. 4.5e-7 / 1.0e-7 .. 4.8e-7 (0.28: d = 128, gb); d = 64: the raw calls' bits
  (e) 1.4e-8 .. 8.7e-7 / 1.4e-8 .. 1.0e-6 (0.41: K = 3, p = 0.1, step 1, layer 2's gW), 60 comparisons; Adam moments at most
      2.09 * 2^-24 of their largest entry, parameters at most 1.01 ulp of theirs
  (f) losses within 3e-7 of the reference's (relative); trajectory: no element outside rtol 1e-4 / atol 1e-6, at most 1.7e-7 off
Value-only breaks of a scratch copy of the library (valid memory, ordinary failures), one run of this file each, tests failing:
  gn_rows ignored in the backward (every row reads gN)           29  ((b) but n = 1, whose row sets all name row 0: NaN off
      the bitmap; all twelve of (e); both of (f))
  the last row slice left out of gW / gb                          15  ((b) at n >= 65 — up to 64 rows are one slice, which the
      break keeps; the two-step tests of (e); both of (f).  The Adam-state tests of (e) are fed the engine's own gradients
      and pass)
  the mask read with the neighbouring feature's bits              19  (all of (a); (b) at p > 0; the two-step tests of (e) at
      p = 0.1)
"""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import gccf_ref64 as ref  # noqa: E402
from tests.test_gpu_ngcf import STREAMS  # noqa: E402  ((seed, stream); the second seed does not fit 32 bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
D = 64


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


@pytest.fixture(scope="module")
def lib(ops):
    from idgrec_amd import native

    return native.lib


@pytest.fixture(scope="module")
def golden_gccf():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "gccf_small.npz"), allow_pickle=False))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rng(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _randn(rng, shape, scale=1.0):
    return dev((rng.standard_normal(shape) * scale).astype(np.float32))


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _p(t, offset=0):
    """Device pointer of a tensor (None: NULL), `offset` floats in."""
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)


def _ok(code, where):
    from idgrec_amd import native

    native.check(code, where)


def _check(what, got, ref64, f32):
    e_k, e_f = ref.errors(got, ref64, f32)
    print("  %-70s e_kernel %.2e  e_f32 %.2e  (%.2f of the band)" % (what, e_k, e_f, e_k / ref.band(e_f)))
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


def _bitmap(n, rows):
    """int32 [ceil(n / 32)] device bitmap with the bits of `rows` set (n % 32 != 0: a partial last word)."""
    rows = np.asarray(rows, dtype=np.int64)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return dev(words.view(np.int32))


def _mask(p, stream, n, d=D, dtype=F64):
    return ref.keep_mask(p, stream[0], stream[1], n, d, dtype=dtype).cuda()


def fwd(ops, lib, side, W, b, p, stream, E, lde, slot=0):
    n = side.shape[0]
    _ok(lib.idg_gccf_layer_fwd_f32(_p(side), _p(W), _p(b), n, D, p, stream[0], stream[1], _p(E, slot), lde, ops._stream()),
        "idg_gccf_layer_fwd_f32")


def bwd(ops, lib, gE, gN, ldgn, bitmap, side, W, p, stream, g_side, w_grads, ws, slot=0):
    n = side.shape[0]
    _ok(lib.idg_gccf_layer_bwd_f32(_p(gE), _p(gN, slot), ldgn, _p(bitmap), _p(side), _p(W), n, D, p, stream[0], stream[1], _p(g_side),
                                   _p(w_grads), _p(ws), ops._stream()), "idg_gccf_layer_bwd_f32")


def _ws(lib):
    return torch.empty(int(lib.idg_gccf_layer_bwd_workspace_bytes(D)) // 4, device="cuda")


# ============================================================================================================ (a) the mask
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mask_is_the_published_one_and_nothing_else_is_written(ops, lib, n):
    """W = I, b = 0, side = 1: the accumulator is exactly 1 (one product 1 * 1 and 63 products 1 * 0), so E IS the keep
    scale or 0.  lde = d, and lde = 4 d into slot 2 of a NaN-filled panel with three rows more than n: every bit outside
    columns 128 .. 191 of rows 0 .. n - 1 is still the NaN it was."""
    W, b, side = torch.eye(D, device="cuda"), torch.zeros(D, device="cuda"), torch.ones(n, D, device="cuda")
    for p in (0.0, 0.1, 0.9):
        for stream in STREAMS:
            want = _mask(p, stream, n, dtype=F32)
            E = _nan(n + 3, D)
            fwd(ops, lib, side, W, b, p, stream, E, D)
            assert torch.equal(E[:n], want), "n=%d p=%g seed=%d: %d elements differ from keep_mask" % (n, p, stream[0], int((E[:n] != want).sum()))
            panel = _nan(n + 3, 4 * D)
            before = panel.view(torch.int32).clone()
            fwd(ops, lib, side, W, b, p, stream, panel, 4 * D, slot=2 * D)
            assert torch.equal(panel[:n, 2 * D:3 * D], want)
            after = panel.view(torch.int32).clone()
            after[:n, 2 * D:3 * D] = before[:n, 2 * D:3 * D]
            assert torch.equal(after, before), "n=%d p=%g: the panel was written outside the slot or past row n - 1" % (n, p)
            assert torch.equal(E.view(torch.int32)[n:], before[n:, :D])
            if p == 0.0:
                assert (want == 1).all()
            elif n >= 63:
                assert abs(float((want == 0).float().mean()) - p) < 0.03


# ======================================================================================= (b) forward and backward vs float64
LAYER_N = [1, 63, 64, 65, 130, 512 * 64 + 65]  # 32,833 rows: 514 blocks on 512 persistent workgroups — two walk a second block


def _row_sets(rng, n):
    """gn_rows: None (every row), a random 5 % (at least one row), and rows 0 and n - 1 only."""
    some = np.unique(rng.choice(n, max(1, n // 20), replace=False))
    return [("all rows", None), ("5% of rows", some), ("rows 0, n-1", np.unique([0, n - 1]))]


def _inputs(key, n, p):
    rng = _rng(key, n, p)
    return rng, _randn(rng, (n, D), 0.3), _randn(rng, (D, D), 0.1), _randn(rng, (D,), 0.1), _randn(rng, (n, D)), _randn(rng, (n, D))


@pytest.mark.parametrize("p", [0.0, 0.1, 0.9])
@pytest.mark.parametrize("n", LAYER_N)
def test_layer_kernels_vs_float64(ops, lib, n, p):
    """n <= 64: one workgroup, one slice; 65, 130: 2 and 3 workgroups, the last with 1 and 2 live rows; 32,833: more tiles than
    the persistent backward grid.  E into slot 2 of a [n, 256] panel; gN from slot 2 of a [n, 256] panel that holds NaN in its
    other slots and off the flagged rows; the workspace holds NaN before each call."""
    rng, side, W, b, gE, gNfull = _inputs("layer", n, p)
    stream = STREAMS[1] if n % 2 else STREAMS[0]
    tag = "n=%d p=%g" % (n, p)
    mask = _mask(p, stream, n)
    panel = torch.full((n, 4 * D), 7.0, device="cuda")
    fwd(ops, lib, side, W, b, p, stream, panel, 4 * D, slot=2 * D)
    assert (panel[:, :2 * D] == 7.0).all() and (panel[:, 3 * D:] == 7.0).all(), tag + ": the panel was written outside the slot"
    E = panel[:, 2 * D:3 * D]
    E64, E32 = ref.layer64(side, W, b, mask), ref.layer64(side, W, b, mask, dtype=F32)
    assert torch.isfinite(E).all()
    _check(tag + " E", E, E64, E32)
    assert torch.equal(E == 0, mask == 0) or p == 0.0, tag + ": E is zero elsewhere than the mask"
    gone = (mask == 0).all(dim=1)
    if p == 0.9 and n > 30000:
        assert 5 <= int(gone.sum()) <= 120  # 0.9^64 = 1.2e-3 of the rows lose every feature
    assert (E[gone] == 0).all()
    Ec = _nan(n, D)
    fwd(ops, lib, side, W, b, p, stream, Ec, D)
    assert torch.equal(Ec, E), tag + ": contiguous E and slot E have other bits"
    ws = _ws(lib)
    for rows_name, rows in _row_sets(rng, n):
        flags = ref._flags(None if rows is None else dev(rows), n, "cuda")
        bitmap = None if rows is None else _bitmap(n, rows)
        gpanel = _nan(n, 4 * D)
        gpanel[:, 2 * D:3 * D] = torch.where(flags[:, None], gNfull, torch.full_like(gNfull, NAN))
        for g_name, ge, use_gn in (("gE", gE, False), ("gN", None, True), ("gE+gN", gE, True)):
            if not use_gn and rows is not None:
                continue  # (gE alone: the bitmap is not read; one run is enough)
            what = "%s %s %s" % (tag, g_name, rows_name)
            gs, wg = _nan(n, D), _nan(D * D + D)
            ws.fill_(NAN)
            bwd(ops, lib, ge, gpanel if use_gn else None, 4 * D, bitmap, side, W, p, stream, gs, wg, ws, slot=2 * D)
            assert torch.isfinite(gs).all(), what + ": NaN from memory that must not be read"
            assert torch.isfinite(wg).all(), what + ": a workspace slice was summed but never written"
            gn = gpanel[:, 2 * D:3 * D] if use_gn else None
            r64 = ref.layer_grads64(side, W, mask, ge, gn, flags)
            r32 = ref.layer_grads64(side, W, mask, ge, gn, flags, dtype=F32)
            assert (gs[gone] == 0).all()
            if float(r64[0].abs().max()) == 0:  # (n = 1, p = 0.9: the one row may keep nothing)
                assert (gs == 0).all() and (wg == 0).all()
                continue
            _check(what + " g_side", gs, r64[1], r32[1])
            _check(what + " gW", wg[:D * D], r64[2][:D * D], r32[2][:D * D])
            _check(what + " gb", wg[D * D:], r64[2][D * D:], r32[2][D * D:])
            if use_gn and rows is None:  # gN from a contiguous panel: same bits
                gs2, wg2 = _nan(n, D), _nan(D * D + D)
                bwd(ops, lib, ge, gNfull.contiguous(), D, None, side, W, p, stream, gs2, wg2, ws)
                assert torch.equal(gs2, gs) and torch.equal(wg2, wg), what + ": contiguous gN and slot gN give other bits"


# ================================================================================================================ (c) run to run
@pytest.mark.parametrize("n", [130, 512 * 64 + 65])
def test_two_runs_give_equal_bits(ops, lib, n):
    p, stream = 0.1, STREAMS[0]
    rng, side, W, b, gE, gN = _inputs("again", n, p)
    bitmap = _bitmap(n, _row_sets(rng, n)[1][1])
    ws = _ws(lib)
    outs = []
    for _ in range(2):
        E, gs, wg = _nan(n, D), _nan(n, D), _nan(D * D + D)
        ws.fill_(NAN)
        fwd(ops, lib, side, W, b, p, stream, E, D)
        bwd(ops, lib, gE, gN, D, bitmap, side, W, p, stream, gs, wg, ws)
        outs.append((E, gs, wg))
    for a, c, name in zip(outs[0], outs[1], ("E", "g_side", "w_grads")):
        assert torch.isfinite(a).all() and torch.equal(a, c), name


# ===================================================================================================== (d) the differentiable path
def test_autograd_at_width_64_is_the_raw_calls_bit_for_bit(ops, lib):
    n, p, stream = 130, 0.1, STREAMS[1]
    rng, side, W, b, gE, _ = _inputs("autograd", n, p)
    s, w, bb = (x.clone().requires_grad_(True) for x in (side, W, b.reshape(1, D)))
    E = ops.gccf_layer(s, w, bb, p, stream=stream)
    E.backward(gE)
    E0, gs, wg = _nan(n, D), _nan(n, D), _nan(D * D + D)
    fwd(ops, lib, side, W, b, p, stream, E0, D)
    bwd(ops, lib, gE, None, D, None, side, W, p, stream, gs, wg, _ws(lib))
    assert torch.equal(E.detach(), E0) and torch.equal(s.grad, gs)
    assert w.grad.shape == (D, D) and bb.grad.shape == (1, D)
    assert torch.equal(w.grad.reshape(-1), wg[:D * D]) and torch.equal(bb.grad.reshape(-1), wg[D * D:])
    # the default stream is the next one of the device seed's sequence: two calls, two masks
    ops.reset_noise_stream()
    a, c = ops.gccf_layer(side, W, b, 0.5), ops.gccf_layer(side, W, b, 0.5)
    assert not torch.equal(a == 0, c == 0)


def test_autograd_at_width_128_vs_float64(ops):
    """No kernel of idg_gccf.hip at this width: tall_linear and ngcf_layer_tail with slope 1 and a zero second bias."""
    n, d, p, stream = 257, 128, 0.1, STREAMS[0]
    rng = _rng("wide", n)
    side, W, b, gE = _randn(rng, (n, d), 0.3), _randn(rng, (d, d), 0.1), _randn(rng, (1, d), 0.1), _randn(rng, (n, d))
    s, w, bb = (x.clone().requires_grad_(True) for x in (side, W, b))
    E = ops.gccf_layer(s, w, bb, p, stream=stream)
    E.backward(gE)
    mask = _mask(p, stream, n, d)
    assert torch.equal(E.detach() == 0, mask == 0)
    _check("d=128 E", E.detach(), ref.layer64(side, W, b, mask), ref.layer64(side, W, b, mask, dtype=F32))
    r64, r32 = ref.layer_grads64(side, W, mask, gE, None), ref.layer_grads64(side, W, mask, gE, None, dtype=F32)
    _check("d=128 g_side", s.grad, r64[1], r32[1])
    _check("d=128 gW", w.grad.reshape(-1), r64[2][:d * d], r32[2][:d * d])
    _check("d=128 gb", bb.grad.reshape(-1), r64[2][d * d:], r32[2][d * d:])


# ================================================================================================================ (e) the engine
REG, LR = float(np.float32(1e-4)), 1e-3
ENGINE_CASES = [(3, 0.0), (3, 0.1), (1, 0.0), (1, 0.1)]
_engine_runs = {}
_graphs = {}


def _graph(ops, golden_small):
    if "g" not in _graphs:
        g = golden_small
        n = int(g["num_users"]) + int(g["num_items"])
        _graphs["g"] = (ops.Graph(g["adjself_indptr"], g["adjself_indices"], g["adjself_data"], n, n),
                        ref.dense_operator(g["adjself_indptr"], g["adjself_indices"], g["adjself_data"], (n, n), device="cuda"))
    return _graphs["g"]


def _engine_run(ops, golden_small, golden_gccf, K, p):
    """Two training steps with store_grad and known dropout streams — the B = 96 batch with duplicate users and items, then a
    256-row one — every step next to step64 in float64 and float32 FROM THE ENGINE'S OWN TABLES read back before the step;
    then the same two steps without store_grad."""
    key = (K, p)
    if key in _engine_runs:
        return _engine_runs[key]
    from idgrec_amd.gccf import GccfEngine

    G, A64 = _graph(ops, golden_small)
    U, I = int(golden_small["num_users"]), int(golden_small["num_items"])
    n = U + I
    rng = _rng("engine", *key)
    xav = lambda r, c: dev(rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32))  # noqa: E731
    P0 = torch.cat([xav(U, D), xav(I, D)])
    small0 = [(xav(D, D), xav(1, D)) for _ in range(K)]
    batches = [tuple(dev(golden_gccf["batch"][:, c]) for c in range(3)),
               tuple(dev(golden_gccf["traj_batches"][256:512, c]) for c in range(3))]  # ([:256] contains the B = 96 batch)
    seeds = [STREAMS[1][0], 77]

    def make(store_grad):
        return GccfEngine(G, U, I, P0.clone(), small0, mess_dropout=[p] * K, reg_lambda=REG, lr=LR, store_grad=store_grad)

    eng = make(True)
    SW0 = eng.SW.clone()
    steps = []
    for s, (users, pos, neg) in enumerate(batches):
        streams = [(seeds[s], l) for l in range(K)]
        P_before = eng.P.clone()
        small_before = [tuple(v.clone() for v in layer) for layer in eng.small_views()]
        loss = eng.train_step(users, pos, neg, streams=streams).clone()
        st = dict(loss=loss, GRAD=eng.GRAD.clone(), SG=eng.SG.clone(), P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(),
                  SW=eng.SW.clone(), SM=eng.SM.clone(), SV=eng.SV.clone(), final=eng.FINAL.clone())
        for name, dtype in (("64", F64), ("32", F32)):
            masks = [_mask(p, sd, n, dtype=dtype) for sd in streams]
            losses, gE0, gsmall, final = ref.step64(A64, P_before, small_before, users, pos, neg, masks, REG, U, dtype=dtype)
            st["loss" + name], st["GRAD" + name], st["final" + name] = losses, gE0, final
            st["SG" + name] = torch.cat([t.reshape(-1) for layer in gsmall for t in layer])
        steps.append(st)
    assert eng.step_count == 2
    lean = make(False)
    for s, (users, pos, neg) in enumerate(batches):
        lean.train_step(users, pos, neg, streams=[(seeds[s], l) for l in range(K)])
    run = dict(P0=P0, SW0=SW0, steps=steps, lean=tuple(t.clone() for t in (lean.P, lean.M, lean.V, lean.SW, lean.SM, lean.SV)))
    torch.cuda.synchronize()
    _engine_runs[key] = run
    return run


@pytest.mark.parametrize("K,p", ENGINE_CASES)
def test_engine_two_steps_vs_float64(ops, golden_small, golden_gccf, K, p):
    """The second step's batch names other rows than the first's: rows of step 1 leaking into step 2 — through the
    regulariser's panel that the last product takes as its masked addend, through GFIN, through the bitmap — would show in
    its table gradient."""
    run = _engine_run(ops, golden_small, golden_gccf, K, p)
    per = D * D + D
    for s, st in enumerate(run["steps"], 1):
        tag = "engine K=%d p=%g step %d" % (K, p, s)
        assert torch.isfinite(st["loss"]).all() and torch.isfinite(st["GRAD"]).all() and torch.isfinite(st["SG"]).all()
        for k, name in enumerate(("bpr", "reg")):
            _check("%s loss %s" % (tag, name), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " final", st["final"], st["final64"], st["final32"])
        _check(tag + " GRAD", st["GRAD"], st["GRAD64"], st["GRAD32"])
        assert torch.equal(st["GRAD"].abs().sum(dim=1) == 0, st["GRAD64"].abs().sum(dim=1) == 0), tag + ": other rows receive gradient"
        for l in range(K):
            for name, lo, hi in (("gW", 0, D * D), ("gb", D * D, per)):
                lo, hi = l * per + lo, l * per + hi
                _check("%s layer %d %s" % (tag, l, name), st["SG"][lo:hi], st["SG64"][lo:hi], st["SG32"][lo:hi])
    # rows of the first batch that the second does not name: what the first step stored there (GFIN, the regulariser's
    # panel) must not reach the second step's gradient — at K = 1 some rows receive gradient in the second step only
    rows = [set(np.concatenate([b[:, 0], 300 + b[:, 1], 300 + b[:, 2]]).tolist())
            for b in (golden_gccf["batch"], golden_gccf["traj_batches"][256:512])]
    assert len(rows[0] - rows[1]) > 20
    if K == 1:
        a, c = (st["GRAD64"].abs().sum(dim=1) > 0 for st in run["steps"])
        assert bool((a & ~c).any()) and bool((c & ~a).any())


@pytest.mark.parametrize("K,p", ENGINE_CASES)
def test_engine_adam_state_after_each_step(ops, golden_small, golden_gccf, K, p):
    """On the embedding panel (Adam in the last product's epilogue) and on the flat buffer of the 2K small tensors (one
    launch): exp_avg, exp_avg_sq within 4 * 2^-24 of their largest entry, the parameters within 4 ulp of their largest entry,
    against the float64 recurrence fed the engine's own two gradients from the float32 initial values."""
    run = _engine_run(ops, golden_small, golden_gccf, K, p)
    for what, W0, gk, wk, mk, vk in (("panel", run["P0"], "GRAD", "P", "M", "V"), ("small", run["SW0"], "SG", "SW", "SM", "SV")):
        want = ref.adam64(W0, [st[gk] for st in run["steps"]], lr=LR)
        for s, (st, (W, M, V)) in enumerate(zip(run["steps"], want), 1):
            for name, got, w in (("exp_avg", st[mk], M), ("exp_avg_sq", st[vk], V)):
                e = float((got.double() - w).abs().max() / w.abs().max())
                print("  K=%d p=%g %s step %d %s: %.2f * 2^-24 of max" % (K, p, what, s, name, e * 2.0 ** 24))
                assert e <= 4 * 2.0 ** -24, (what, name, s, e)
            wmax = float(W.abs().max())
            ulp = float(np.spacing(np.float32(wmax)))
            e = float((st[wk].double() - W).abs().max())
            print("  K=%d p=%g %s step %d parameters: %.2f ulp of max |W| = %.3f" % (K, p, what, s, e / ulp, wmax))
            assert e <= 4 * ulp, (what, s, e / ulp)
        assert not torch.equal(run["steps"][0][wk], run["steps"][1][wk])


@pytest.mark.parametrize("K,p", ENGINE_CASES)
def test_engine_without_stored_gradient_is_bit_identical(ops, golden_small, golden_gccf, K, p):
    run = _engine_run(ops, golden_small, golden_gccf, K, p)
    last = run["steps"][-1]
    for got, name in zip(run["lean"], ("P", "M", "V", "SW", "SM", "SV")):
        assert torch.equal(got, last[name]), name


# ================================================================================================================ (f) the plugin
def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "GCCF.txt"), "GCCF")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _data(tmp_path, g, name, cfg):
    import utility.utility_data.data_loader as data_loader

    d = tmp_path / name
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset=name, dataset_path=str(tmp_path) + "/", sparsity_test="0")
    return data_loader.Data(str(d), cfg)


@pytest.mark.parametrize("tag,K", [("def", 3), ("one", 1)])
def test_model_matches_reference_goldens(ops, tag, K, tmp_path, golden_small, golden_gccf):
    import utility.utility_function.tools as tools
    from models.GCCF import GCCF

    g = golden_gccf
    cfg = _cfg(mess_drop_prob="[0.0, 0.0, 0.0]", GCN_layer=K)  # the goldens were taken with message dropout off
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = GCCF(cfg, data, torch.device("cuda")).to("cuda")
    assert np.array_equal(m.user_embedding.weight.detach().cpu().numpy(), g["init_user"])
    assert np.array_equal(m.item_embedding.weight.detach().cpu().numpy(), g["init_item"])
    names = [nm % l for l in range(K) for nm in ("W_gcn_%d", "b_gcn_%d")]
    assert list(m.weight_dict.keys()) == names and len(list(m.parameters())) == 2 + 2 * K
    for nm in names:  # same torch RNG order as the reference's constructor
        assert np.array_equal(m.weight_dict[nm].detach().cpu().numpy(), g["%s_%s" % (tag, nm)]), nm
    b = torch.from_numpy(g["batch"]).cuda()
    au, ai = m.aggregate()
    assert au.shape == (data.num_users, 64 * (K + 1)) and ai.shape == (data.num_items, 64 * (K + 1))
    m.zero_grad()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 2
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-4)
    sum(ll).backward()
    np.testing.assert_allclose(m.user_embedding.weight.grad.cpu().numpy(), g[tag + "_grad_user"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(m.item_embedding.weight.grad.cpu().numpy(), g[tag + "_grad_item"], rtol=1e-3, atol=1e-8)
    for nm in names:
        np.testing.assert_allclose(m.weight_dict[nm].grad.cpu().numpy(), g["%s_grad_%s" % (tag, nm)], rtol=1e-3, atol=1e-7)
    m.eval()
    users = torch.from_numpy(g["rating_users"]).cuda()
    np.testing.assert_allclose(m.get_rating_for_test(users).cpu().numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    assert m.topk_for_test(users, 10).shape == (32, 10)
    # three fused steps against the reference's own Adam trajectory
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    tools.set_seed(2024)
    m = GCCF(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 2), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    # (the trajectory criterion of tests/test_gpu_lgcnpp.py: Adam divides by sqrt(v), so where a gradient is of the order of
    # its own rounding error a last-place difference moves the element visibly)
    pairs = [(m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])]
    pairs += [(m.weight_dict[nm], g["%s_traj_%s" % (tag, nm)]) for nm in names]
    for mine, want in pairs:
        mine = mine.detach().cpu().numpy()
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("trajectory: off %.3g, max %.3g" % (off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - want).max() < 1e-4, np.abs(mine - want).max()
    assert all(int(opt.state[prm]["step"]) == 3 for prm in m.parameters())


def test_model_paths_that_do_not_fuse(ops, tmp_path, golden_small):
    """layer_size that is not [d] * K, and node dropout: the differentiable path only; both give finite losses and a gradient
    for every parameter."""
    import utility.utility_function.tools as tools
    from models.GCCF import GCCF

    rng = _rng("batch")
    b = [dev(rng.integers(0, hi, 128).astype(np.int64)) for hi in (300, 250, 250)]
    for extra in (dict(layer_size="[128, 64, 32]"), dict(node_dropout=True, node_keep_prob=0.9)):
        cfg = _cfg(**extra)
        data = _data(tmp_path, golden_small, "small", cfg)
        tools.set_seed(2024)
        m = GCCF(cfg, data, torch.device("cuda")).to("cuda")
        assert not m.fused_step_available()
        m.train()
        ll = m(*b)
        sum(ll).backward()
        assert all(torch.isfinite(x).all() for x in ll)
        for name, prm in m.named_parameters():
            assert prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0, name
        au, ai = m.aggregate()
        assert au.shape[1] == 64 + sum(eval(cfg["layer_size"]))
