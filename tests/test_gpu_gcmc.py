"""GCMC's layer kernels (idgrec_amd/csrc/idg_gcmc.hip), their differentiable wrapper (ops.gcmc_layer), the fused step
(idgrec_amd/gcmc.py) and the plugin (models/GCMC.py) on the device.  The reference statement is tests/gcmc_ref64.py, pinned to
the reference's own numbers by tests/test_gcmc_host.py.

  (a) the message-dropout mask of the forward kernel, bit for bit against ngcf_ref64.keep_mask, and untouched memory;
  (b) idg_gcmc_layer_fwd_f32 / idg_gcmc_layer_bwd_f32 against float64: 1, 2, 3 and more than 512 blocks, gE / gN / both,
      no bitmap / a 5 % bitmap / first and last row only, N written into and gN read from a slot of a wider panel, NaN in
      unread memory; exact zeros of H; a panel below the normalisation clamp;
  (c) run to run: two calls give equal bits, the parameter gradients included;
  (d) ops.gcmc_layer under autograd: the raw calls' bits at d = 64, the composition of existing operators at d = 128;
  (e) GcmcEngine, two consecutive steps with different batches: losses, every gradient, Adam state, parameters;
  (f) models.GCMC against the reference's goldens (tests/golden/gcmc_small.npz): losses, gradients, rating, trajectory;
  (g) the hand-off of an optimizer's Adam state to the engine (what tests/test_gpu_engine_handoff.py asks of the others).

One tolerance rule throughout (b), (d), (e) (egcf_ref64.errors / band): with scale = max |ref64| of the tensor compared,
    e_kernel = max |kernel - ref64| / scale   <=   max(4 e_f32, 8 * 2^-24),   e_f32 = max |float32 composition - ref64| / scale
where the float32 composition is gcmc_ref64's same expressions in float32, run in the same test; both numbers are printed
(pytest -s).  Rows next to LeakyReLU's kink — an element of the float64 H with 0 < |H| < 1e-5 * (|side| . |Wg| + |bg|),
tests/test_gpu_ngcf.py::_near_the_kink's rule — get zero upstream gradient in (b) and (d): a float32 H may land on the other
side there in ANY correct evaluation.  They must be at most 1 % of the rows (asserted).  Counted on the CPU from gcmc_ref64 for the inputs of (b): none at
n <= 130, and 78, 84 and 83 of 32,833 rows (0.24 .. 0.26 %) at p = 0, 0.1, 0.9; the share by hand was 0.3 %.
Kernel and reference share the graph's float32 values (dense_operator), the mask and its float32 scale (keep_mask) and the
float32 rounding of reg_lambda.  The Adam state of (e) follows tests/test_gpu_gccf.py::test_engine_adam_state_after_each_step;
(f) uses the tolerances of tests/test_gpu_gccf.py::test_model_matches_reference_goldens.

Measured on an MI355X (47 tests, 6 .. 7 s for the whole file once the library is loaded), e_kernel / e_f32 over all
comparisons of a group, worst e_kernel / band:
  (a) exact: every T equals keep_mask bit for bit, N within 4 * 2^-24 of T / |T|, every other bit of both panels is the NaN it
      was (5 tests, 30 panel pairs)
  (b) 0 .. 2.0e-5 / 0 .. 3.3e-5 (0.66: n = 32,833, p = 0.9, gN at 5 % of the rows, g_side; the largest errors at p = 0.9, where
      a row's norm rests on a few elements), 666 comparisons.  n = 1, p = 0.9 — the one row keeps six elements — at most 0.42
      (gWm); its T: 3.0e-7 / 2.0e-7 (0.38).  With each product summed as ONE chain of 32 MFMA steps that T sat at 8.4e-7, 1.07 of
      the band, and the case failed: the kernels now sum two (H) and four (M) chains pairwise (idg_gcmc.hip, tile_times_w)
      exact zeros of H: 5.8e-8 .. 3.8e-7 / 5.9e-8 .. 5.7e-7 (0.48: p = 0.1, gN at rows 0 and n - 1, gbg), 74 comparisons
      rows below the clamp: 0 .. 3.3e-7 / 0 .. 4.2e-7 (0.34: p = 0.1, gbm, of the order 1e12), 16 comparisons; g_side, gWg, gbg
      exactly 0 and N == T / 1e-12 bit for bit
  (d) 1.1e-7 .. 4.3e-7 / 1.1e-7 .. 6.8e-7 (0.28: d = 128, g_side); d = 64: the raw calls' bits
  (e) 1.8e-9 .. 1.4e-5 / 1.8e-9 .. 1.8e-5 (0.71: K = 2, p = 0.1, step 2, layer 1's gbm), 80 comparisons; Adam moments at most
      2.05 * 2^-24 of their largest entry, parameters at most 0.99 ulp of theirs
  (f) losses within 2e-7 of the reference's (relative); trajectory: no element outside rtol 1e-4 / atol 1e-6
Value-only breaks of a scratch copy of the library (valid memory, ordinary failures), one run of this file each, tests failing:
  gn_rows ignored in the backward (every row reads gN)           33  ((b) but n = 1, whose row sets all name row 0: NaN off
      the bitmap; the constructed cases; all twelve of (e); both of (f))
  the last row slice left out of the reduction                    19  ((b) at n >= 65 — up to 64 rows are one slice, which the
      break keeps; the constructed cases (n = 130); the two-step tests of (e); both of (f).  The Adam-state tests of (e) are
      fed the engine's own gradients and pass)
  LeakyReLU' taken as 1 everywhere                                26  (all of (b); the exact zeros; the two-step tests of (e);
      both of (f).  The rows below the clamp pass: with Wm = 0 nothing reaches the activation)
"""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import gcmc_ref64 as ref  # noqa: E402
from tests.test_gpu_ngcf import KINK, STREAMS, _near_the_kink  # noqa: E402  ((seed, stream); the second seed does not fit 32 bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
D = 64
WW = D * D
HALF = WW + D
SLOPE = 0.2
NAMES = ("W_gcn_%d", "b_gcn_%d", "W_mlp_%d", "b_mlp_%d")
PARTS = (("gWg", 0, WW), ("gbg", WW, HALF), ("gWm", HALF, HALF + WW), ("gbm", HALF + WW, 2 * HALF))
BWD_GRID = 512  # persistent workgroups of the backward kernel


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
def golden_gcmc():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "gcmc_small.npz"), allow_pickle=False))


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


def fwd(ops, lib, side, Wg, bg, Wm, bm, p, stream, T, N, ldn, slot=0):
    n = side.shape[0]
    _ok(lib.idg_gcmc_layer_fwd_f32(_p(side), _p(Wg), _p(bg), _p(Wm), _p(bm), n, D, SLOPE, p, stream[0], stream[1], _p(T),
                                   _p(N, slot), ldn, ops._stream()), "idg_gcmc_layer_fwd_f32")


def bwd(ops, lib, T, gE, gN, ldgn, bitmap, side, Wg, bg, Wm, p, stream, g_side, w_grads, ws, slot=0):
    n = side.shape[0]
    _ok(lib.idg_gcmc_layer_bwd_f32(_p(T), _p(gE), _p(gN, slot), ldgn, _p(bitmap), _p(side), _p(Wg), _p(bg), _p(Wm), n, D, SLOPE, p,
                                   stream[0], stream[1], _p(g_side), _p(w_grads), _p(ws), ops._stream()), "idg_gcmc_layer_bwd_f32")


def _ws(lib):
    return torch.empty(int(lib.idg_gcmc_layer_bwd_workspace_bytes(D)) // 4, device="cuda")


# ============================================================================================================ (a) the mask
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mask_is_the_published_one_and_nothing_else_is_written(ops, lib, n):
    """Wg = Wm = I, biases 0, side = 1: both accumulators are exactly 1 (one product 1 * 1 and 63 products 1 * 0) and
    LeakyReLU(1) = 1, so T IS the keep scale or 0.  N goes into slot 2 of a NaN-filled [n + 3, 256] panel, T into a NaN-filled
    [n + 3, 64] one: every bit outside columns 128 .. 191 of rows 0 .. n - 1 of the first, and past row n - 1 of the second,
    is still the NaN it was."""
    eye, zero, side = torch.eye(D, device="cuda"), torch.zeros(D, device="cuda"), torch.ones(n, D, device="cuda")
    for p in (0.0, 0.1, 0.9):
        for stream in STREAMS:
            want = _mask(p, stream, n, dtype=F32)
            T, panel = _nan(n + 3, D), _nan(n + 3, 4 * D)
            t_before, before = T.view(torch.int32).clone(), panel.view(torch.int32).clone()
            fwd(ops, lib, side, eye, zero, eye, zero, p, stream, T, panel, 4 * D, slot=2 * D)
            assert torch.equal(T[:n], want), "n=%d p=%g seed=%d: %d elements differ from keep_mask" % (n, p, stream[0], int((T[:n] != want).sum()))
            assert torch.equal(T.view(torch.int32)[n:], t_before[n:]), "n=%d p=%g: T was written past row n - 1" % (n, p)
            N = panel[:n, 2 * D:3 * D]
            den = want.double().pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
            assert torch.isfinite(N).all() and torch.equal(N == 0, want == 0)
            assert float((N.double() - want.double() / den).abs().max()) <= 4 * 2.0 ** -24  # (|N| <= 1)
            after = panel.view(torch.int32).clone()
            after[:n, 2 * D:3 * D] = before[:n, 2 * D:3 * D]
            assert torch.equal(after, before), "n=%d p=%g: the panel was written outside the slot or past row n - 1" % (n, p)
            if p == 0.0:
                assert (want == 1).all()
            elif n >= 63:
                assert abs(float((want == 0).float().mean()) - p) < 0.03


# ======================================================================================= (b) forward and backward vs float64
LAYER_N = [1, 63, 64, 65, 130, BWD_GRID * 64 + 65]  # 32,833 rows: 514 blocks on 512 persistent workgroups — two walk a second block
INPUT_KEY = "gcmc-layer-1"  # (the first key tried, "gcmc-layer", puts one to three of 63 .. 130 rows next to the kink: over the cap)


def _row_sets(rng, n):
    """gn_rows: None (every row), a random 5 % (at least one row), and rows 0 and n - 1 only."""
    some = np.unique(rng.choice(n, max(1, n // 20), replace=False))
    return [("all rows", None), ("5% of rows", some), ("rows 0, n-1", np.unique([0, n - 1]))]


def _inputs(key, n, p, d=D):
    """tests/test_gpu_gccf.py::_inputs' scales: side 0.3, weights and biases 0.1, upstream gradients 1."""
    rng = _rng(key, n, p)
    return (rng, _randn(rng, (n, d), 0.3), _randn(rng, (d, d), 0.1), _randn(rng, (d,), 0.1), _randn(rng, (d, d), 0.1),
            _randn(rng, (d,), 0.1), _randn(rng, (n, d)), _randn(rng, (n, d)))


def _kink_rows(tag, side, Wg, bg):
    """Rows next to LeakyReLU's kink, from the float64 H alone; at most 1 % of the rows (a condition on the inputs)."""
    kink = _near_the_kink(ref.hidden64(side, Wg, bg), ref.hidden64(side.abs(), Wg.abs(), bg.abs()))
    print("  %s: %d of %d rows next to the kink (KINK = %g) carry no upstream gradient" % (tag, int(kink.sum()), side.shape[0], KINK))
    assert int(kink.sum()) <= 0.01 * side.shape[0], tag + ": more than 1 % of the rows next to the kink: change the input key"
    return kink


def _layer_case(ops, lib, tag, n, p, stream, rng, side, Wg, bg, Wm, bm, gE, gNfull, variants=None, own_scale=False):
    """Forward into a slot and contiguous, then every (upstream, bitmap) combination of the backward, against float64."""
    mask = _mask(p, stream, n)
    kink = _kink_rows(tag, side, Wg, bg)
    gE, gNfull = gE.clone(), gNfull.clone()
    gE[kink], gNfull[kink] = 0.0, 0.0
    panel = torch.full((n, 4 * D), 7.0, device="cuda")
    T = _nan(n, D)
    fwd(ops, lib, side, Wg, bg, Wm, bm, p, stream, T, panel, 4 * D, slot=2 * D)
    assert (panel[:, :2 * D] == 7.0).all() and (panel[:, 3 * D:] == 7.0).all(), tag + ": the panel was written outside the slot"
    N = panel[:, 2 * D:3 * D]
    (T64, N64), (T32, N32) = ref.layer64(side, Wg, bg, Wm, bm, mask), ref.layer64(side, Wg, bg, Wm, bm, mask, dtype=F32)
    assert torch.isfinite(T).all() and torch.isfinite(N).all()
    _check(tag + " T", T, T64, T32)
    _check(tag + " N", N, N64, N32)
    assert torch.equal(T == 0, mask == 0) or p == 0.0, tag + ": T is zero elsewhere than the mask"
    gone = (mask == 0).all(dim=1)
    assert (T[gone] == 0).all() and (N[gone] == 0).all()
    Tc, Nc = _nan(n, D), _nan(n, D)
    fwd(ops, lib, side, Wg, bg, Wm, bm, p, stream, Tc, Nc, D)
    assert torch.equal(Tc, T) and torch.equal(Nc, N), tag + ": contiguous N and slot N have other bits"
    ws = _ws(lib)
    for rows_name, rows in _row_sets(rng, n):
        flags = ref._flags(None if rows is None else dev(rows), n, "cuda")
        bitmap = None if rows is None else _bitmap(n, rows)
        gpanel = _nan(n, 4 * D)
        gpanel[:, 2 * D:3 * D] = torch.where(flags[:, None], gNfull, torch.full_like(gNfull, NAN))
        for g_name, ge, use_gn in (("gE", gE, False), ("gN", None, True), ("gE+gN", gE, True)):
            if (not use_gn and rows is not None) or (variants is not None and g_name not in variants):
                continue  # (gE alone: the bitmap is not read; one run is enough)
            what = "%s %s %s" % (tag, g_name, rows_name)
            gs, wg = _nan(n, D), _nan(2 * HALF)
            ws.fill_(NAN)
            bwd(ops, lib, T, ge, gpanel if use_gn else None, 4 * D, bitmap, side, Wg, bg, Wm, p, stream, gs, wg, ws, slot=2 * D)
            assert torch.isfinite(gs).all(), what + ": NaN from memory that must not be read"
            assert torch.isfinite(wg).all(), what + ": a workspace slice was summed but never written"
            gn = gpanel[:, 2 * D:3 * D] if use_gn else None
            r64 = ref.layer_grads64(side, Wg, bg, Wm, bm, mask, ge, gn, flags)
            r32 = ref.layer_grads64(side, Wg, bg, Wm, bm, mask, ge, gn, flags, dtype=F32)
            assert (gs[gone] == 0).all() and (gs[kink] == 0).all()
            if float(r64[1].abs().max()) == 0:  # (n = 1, p = 0.9: the one row may keep nothing)
                assert (gs == 0).all() and (wg == 0).all()
                continue
            if own_scale:  # Wm = 0: nothing flows past the second product
                assert (gs == 0).all() and (wg[:HALF] == 0).all() and float(r64[0].abs().max()) == 0
            else:
                _check(what + " g_side", gs, r64[0], r32[0])
            for name, lo, hi in PARTS[2:] if own_scale else PARTS:
                _check("%s %s" % (what, name), wg[lo:hi], r64[1][lo:hi], r32[1][lo:hi])
            if use_gn and rows is None:  # gN from a contiguous panel: same bits
                gs2, wg2 = _nan(n, D), _nan(2 * HALF)
                bwd(ops, lib, T, ge, gNfull.contiguous(), D, None, side, Wg, bg, Wm, p, stream, gs2, wg2, ws)
                assert torch.equal(gs2, gs) and torch.equal(wg2, wg), what + ": contiguous gN and slot gN give other bits"
    return T, N


@pytest.mark.parametrize("p", [0.0, 0.1, 0.9])
@pytest.mark.parametrize("n", LAYER_N)
def test_layer_kernels_vs_float64(ops, lib, n, p):
    """n <= 64: one workgroup, one slice; 65, 130: 2 and 3 workgroups, the last with 1 and 2 live rows; 32,833: more tiles than
    the persistent backward grid.  N into slot 2 of a [n, 256] panel; gN from slot 2 of a [n, 256] panel that holds NaN in its
    other slots and off the flagged rows; the workspace holds NaN before each call."""
    rng, side, Wg, bg, Wm, bm, gE, gN = _inputs(INPUT_KEY, n, p)
    stream = STREAMS[1] if n % 2 else STREAMS[0]
    T, _ = _layer_case(ops, lib, "n=%d p=%g" % (n, p), n, p, stream, rng, side, Wg, bg, Wm, bm, gE, gN)
    if p == 0.9 and n > 30000:
        assert 5 <= int((T == 0).all(dim=1).sum()) <= 120  # 0.9^64 = 1.2e-3 of the rows lose every feature


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_exact_zeros_of_the_hidden_layer(ops, lib, p):
    """Wg = I and side = -bg on a third of the elements: H is exactly 0 there in float32 and in float64 (one product by 1 and
    63 by 0, then -bg + bg), the kink rule does not exempt an exact zero, and kernel and torch must agree on the slope."""
    n = 130
    rng, side, _, bg, Wm, bm, gE, gN = _inputs("zeros", n, p)
    at = dev(rng.random((n, D)) < 1.0 / 3)
    side = torch.where(at, -bg.reshape(1, D).expand(n, D), side)
    Wg = torch.eye(D, device="cuda")
    assert (ref.hidden64(side, Wg, bg)[at] == 0).all() and (ref.hidden64(side, Wg, bg, dtype=F32)[at] == 0).all()
    assert 0.25 < float(at.float().mean()) < 0.42
    _layer_case(ops, lib, "H = 0 p=%g" % p, n, p, STREAMS[0], rng, side, Wg, bg, Wm, bm, gE, gN)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_rows_below_the_normalisation_clamp(ops, lib, p):
    """Wm = 0, bm = +-1e-13: every row of T has the norm 8e-13 or less — below the clamp, not zero — so N = T / 1e-12 and
    the Jacobian is I / 1e-12: gWm and gbm are of the order 1e12 and compared on their own scale; nothing flows past Wm."""
    n = 130
    rng, side, Wg, bg, _, _, gE, gN = _inputs("clamp", n, p)
    Wm = torch.zeros(D, D, device="cuda")
    bm = dev(np.where(rng.random(D) < 0.5, -1e-13, 1e-13).astype(np.float32))
    T, N = _layer_case(ops, lib, "clamped p=%g" % p, n, p, STREAMS[1], rng, side, Wg, bg, Wm, bm, gE, gN, variants=("gN",), own_scale=True)
    assert float(T.abs().max()) <= 1.2e-13 and float(T.norm(dim=1).max()) < 1e-12 and float(T.abs().max()) > 0
    assert torch.equal(N, T / torch.full_like(T, 1e-12))  # (a tensor divisor: a true division, as the kernel's)


# ================================================================================================================ (c) run to run
@pytest.mark.parametrize("n", [130, BWD_GRID * 64 + 65])
def test_two_runs_give_equal_bits(ops, lib, n):
    p, stream = 0.1, STREAMS[0]
    rng, side, Wg, bg, Wm, bm, gE, gN = _inputs("again", n, p)
    bitmap = _bitmap(n, _row_sets(rng, n)[1][1])
    ws = _ws(lib)
    outs = []
    for _ in range(2):
        T, N, gs, wg = _nan(n, D), _nan(n, D), _nan(n, D), _nan(2 * HALF)
        ws.fill_(NAN)
        fwd(ops, lib, side, Wg, bg, Wm, bm, p, stream, T, N, D)
        bwd(ops, lib, T, gE, gN, D, bitmap, side, Wg, bg, Wm, p, stream, gs, wg, ws)
        outs.append((T, N, gs, wg))
    for a, c, name in zip(outs[0], outs[1], ("T", "N", "g_side", "w_grads")):
        assert torch.isfinite(a).all() and torch.equal(a, c), name


# ===================================================================================================== (d) the differentiable path
def test_autograd_at_width_64_is_the_raw_calls_bit_for_bit(ops, lib):
    n, p, stream = 130, 0.1, STREAMS[1]
    rng, side, Wg, bg, Wm, bm, gE, gN = _inputs("autograd", n, p)
    leaves = [x.clone().requires_grad_(True) for x in (side, Wg, bg.reshape(1, D), Wm, bm.reshape(1, D))]
    T, N = ops.gcmc_layer(*leaves, p, stream=stream)
    torch.autograd.backward([T, N], [gE, gN])
    T0, N0, gs, wg = _nan(n, D), _nan(n, D), _nan(n, D), _nan(2 * HALF)
    fwd(ops, lib, side, Wg, bg, Wm, bm, p, stream, T0, N0, D)
    bwd(ops, lib, T0, gE, gN, D, None, side, Wg, bg, Wm, p, stream, gs, wg, _ws(lib))
    assert torch.equal(T.detach(), T0) and torch.equal(N.detach(), N0) and torch.equal(leaves[0].grad, gs)
    assert [tuple(x.grad.shape) for x in leaves[1:]] == [(D, D), (1, D), (D, D), (1, D)]
    for x, (name, lo, hi) in zip(leaves[1:], PARTS):
        assert torch.equal(x.grad.reshape(-1), wg[lo:hi]), name
    # the default stream is the next one of the device seed's sequence: two calls, two masks
    ops.reset_noise_stream()
    a, c = ops.gcmc_layer(side, Wg, bg, Wm, bm, 0.5)[0], ops.gcmc_layer(side, Wg, bg, Wm, bm, 0.5)[0]
    assert not torch.equal(a == 0, c == 0)


def test_autograd_at_width_128_vs_float64(ops):
    """No kernel of idg_gcmc.hip at this width: tall_linear and ngcf_layer_tail twice (the activation, then the mask and the
    row norm)."""
    n, d, p, stream = 257, 128, 0.1, STREAMS[0]
    rng, side, Wg, bg, Wm, bm, gE, gN = _inputs("wide", n, p, d)
    kink = _kink_rows("d=128", side, Wg, bg)
    gE[kink], gN[kink] = 0.0, 0.0
    leaves = [x.clone().requires_grad_(True) for x in (side, Wg, bg.reshape(1, d), Wm, bm.reshape(1, d))]
    T, N = ops.gcmc_layer(*leaves, p, stream=stream)
    torch.autograd.backward([T, N], [gE, gN])
    mask = _mask(p, stream, n, d)
    assert torch.equal(T.detach() == 0, mask == 0)
    (T64, N64), (T32, N32) = ref.layer64(side, Wg, bg, Wm, bm, mask), ref.layer64(side, Wg, bg, Wm, bm, mask, dtype=F32)
    _check("d=128 T", T.detach(), T64, T32)
    _check("d=128 N", N.detach(), N64, N32)
    r64 = ref.layer_grads64(side, Wg, bg, Wm, bm, mask, gE, gN)
    r32 = ref.layer_grads64(side, Wg, bg, Wm, bm, mask, gE, gN, dtype=F32)
    _check("d=128 g_side", leaves[0].grad, r64[0], r32[0])
    got = torch.cat([x.grad.reshape(-1) for x in leaves[1:]])
    h = d * d + d
    for name, lo, hi in (("gWg", 0, d * d), ("gbg", d * d, h), ("gWm", h, h + d * d), ("gbm", h + d * d, 2 * h)):
        _check("d=128 " + name, got[lo:hi], r64[1][lo:hi], r32[1][lo:hi])


# ================================================================================================================ (e) the engine
REG, LR = float(np.float32(1e-4)), 1e-3
ENGINE_CASES = [(1, 0.0), (1, 0.1), (2, 0.0), (2, 0.1)]
_engine_runs = {}
_graphs = {}


def _graph(ops, golden_small):
    if "g" not in _graphs:
        g = golden_small
        n = int(g["num_users"]) + int(g["num_items"])
        _graphs["g"] = (ops.Graph(g["adj_indptr"], g["adj_indices"], g["adj_data"], n, n),
                        ref.dense_operator(g["adj_indptr"], g["adj_indices"], g["adj_data"], (n, n), device="cuda"))
    return _graphs["g"]


def _engine_run(ops, golden_small, golden_gcmc, K, p):
    """Two training steps with store_grad and known dropout streams — the B = 96 batch with duplicate users and items, then a
    256-row one — every step next to step64 in float64 and float32 FROM THE ENGINE'S OWN TABLES read back before the step;
    then the same two steps without store_grad."""
    key = (K, p)
    if key in _engine_runs:
        return _engine_runs[key]
    from idgrec_amd.gcmc import GcmcEngine

    G, A64 = _graph(ops, golden_small)
    U, I = int(golden_small["num_users"]), int(golden_small["num_items"])
    n = U + I
    rng = _rng("engine", *key)
    xav = lambda r, c: dev(rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32))  # noqa: E731
    P0 = torch.cat([xav(U, D), xav(I, D)])
    small0 = [(xav(D, D), xav(1, D), xav(D, D), xav(1, D)) for _ in range(K)]
    batches = [tuple(dev(golden_gcmc["batch"][:, c]) for c in range(3)),
               tuple(dev(golden_gcmc["traj_batches"][256:512, c]) for c in range(3))]  # ([:256] contains the B = 96 batch)
    seeds = [STREAMS[1][0], 77]

    def make(store_grad):
        return GcmcEngine(G, U, I, P0.clone(), small0, mess_dropout=[p] * K, reg_lambda=REG, lr=LR, store_grad=store_grad)

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
def test_engine_two_steps_vs_float64(ops, golden_small, golden_gcmc, K, p):
    """The second step's batch names other rows than the first's: rows of step 1 leaking into step 2 — through the
    regulariser's panel that the last product takes as its masked addend, through GFIN, through the bitmap — would show in
    its table gradient."""
    run = _engine_run(ops, golden_small, golden_gcmc, K, p)
    for s, st in enumerate(run["steps"], 1):
        tag = "engine K=%d p=%g step %d" % (K, p, s)
        assert torch.isfinite(st["loss"]).all() and torch.isfinite(st["GRAD"]).all() and torch.isfinite(st["SG"]).all()
        for k, name in enumerate(("bpr", "reg")):
            _check("%s loss %s" % (tag, name), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " final", st["final"], st["final64"], st["final32"])
        _check(tag + " GRAD", st["GRAD"], st["GRAD64"], st["GRAD32"])
        assert torch.equal(st["GRAD"].abs().sum(dim=1) == 0, st["GRAD64"].abs().sum(dim=1) == 0), tag + ": other rows receive gradient"
        for l in range(K):
            for name, lo, hi in PARTS:
                lo, hi = l * 2 * HALF + lo, l * 2 * HALF + hi
                _check("%s layer %d %s" % (tag, l, name), st["SG"][lo:hi], st["SG64"][lo:hi], st["SG32"][lo:hi])
    rows = [set(np.concatenate([b[:, 0], 300 + b[:, 1], 300 + b[:, 2]]).tolist())
            for b in (golden_gcmc["batch"], golden_gcmc["traj_batches"][256:512])]
    assert len(rows[0] - rows[1]) > 20
    if K == 1:
        a, c = (st["GRAD64"].abs().sum(dim=1) > 0 for st in run["steps"])
        assert bool((a & ~c).any()) and bool((c & ~a).any())


@pytest.mark.parametrize("K,p", ENGINE_CASES)
def test_engine_adam_state_after_each_step(ops, golden_small, golden_gcmc, K, p):
    """tests/test_gpu_gccf.py's rule: exp_avg, exp_avg_sq within 4 * 2^-24 of their largest entry, the parameters within 4 ulp
    of their largest entry, against the float64 recurrence fed the engine's own two gradients from the float32 initial values."""
    run = _engine_run(ops, golden_small, golden_gcmc, K, p)
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
def test_engine_without_stored_gradient_is_bit_identical(ops, golden_small, golden_gcmc, K, p):
    run = _engine_run(ops, golden_small, golden_gcmc, K, p)
    last = run["steps"][-1]
    for got, name in zip(run["lean"], ("P", "M", "V", "SW", "SM", "SV")):
        assert torch.equal(got, last[name]), name


# ================================================================================================================ (f) the plugin
def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "GCMC.txt"), "GCMC")
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


@pytest.mark.parametrize("tag,K", [("def", 1), ("two", 2)])
def test_model_matches_reference_goldens(ops, tag, K, tmp_path, golden_small, golden_gcmc):
    import utility.utility_function.tools as tools
    from models.GCMC import GCMC

    g = golden_gcmc
    cfg = _cfg(mess_drop_prob="[0.0, 0.0, 0.0]", GCN_layer=K)  # the goldens were taken with message dropout off
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = GCMC(cfg, data, torch.device("cuda")).to("cuda")
    assert np.array_equal(m.user_embedding.weight.detach().cpu().numpy(), g["init_user"])
    assert np.array_equal(m.item_embedding.weight.detach().cpu().numpy(), g["init_item"])
    names = [nm % l for l in range(K) for nm in NAMES]
    assert list(m.weight_dict.keys()) == names and len(list(m.parameters())) == 2 + 4 * K
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
    m = GCMC(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 2), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    pairs = [(m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])]
    pairs += [(m.weight_dict[nm], g["%s_traj_%s" % (tag, nm)]) for nm in names]
    for mine, want in pairs:
        mine = mine.detach().cpu().numpy()
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("trajectory: off %.3g, max %.3g" % (off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - want).max() < 1e-4, np.abs(mine - want).max()
    assert all(int(opt.state[prm]["step"]) == 3 for prm in m.parameters())


def test_model_path_that_does_not_fuse(ops, tmp_path, golden_small):
    """layer_size = [128, 64] with two layers: the differentiable path only (rectangular layers: the composition of existing
    operators, then the 64 x 64 kernels); finite losses and a gradient for every parameter."""
    import utility.utility_function.tools as tools
    from models.GCMC import GCMC

    rng = _rng("batch")
    b = [dev(rng.integers(0, hi, 128).astype(np.int64)) for hi in (300, 250, 250)]
    cfg = _cfg(layer_size="[128, 64]", GCN_layer=2)
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = GCMC(cfg, data, torch.device("cuda")).to("cuda")
    assert not m.fused_step_available() and len(list(m.parameters())) == 10
    m.train()
    ll = m(*b)
    sum(ll).backward()
    assert all(torch.isfinite(x).all() for x in ll)
    for name, prm in m.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0, name
    au, ai = m.aggregate()
    assert au.shape[1] == ai.shape[1] == 64 + 128 + 64
    loss = torch.zeros(2, device="cuda")
    assert m.fused_train_step(*b, loss, ops.Adam(m.parameters(), lr=1e-3)) is False


# ================================================================================================================ (g) the hand-off
def _handoff_model(tmp_path, g):
    import utility.utility_function.tools as tools
    from models.GCMC import GCMC

    cfg = _cfg(mess_drop_prob="[0.0, 0.0, 0.0]", GCN_layer=2)
    data = _data(tmp_path, g, "small", cfg)
    tools.set_seed(2024)
    m = GCMC(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available()
    params = list(m.parameters())
    assert len(params) == 2 + 8
    tri = torch.from_numpy(g["sample1"][:3 * 256]).cuda()
    batches = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(3)]
    return m, params, batches, torch.zeros(m.n_fused_losses, device="cuda")


def test_adam_state_hand_off(ops, tmp_path, golden_small):
    """tests/test_gpu_engine_handoff.py's three requirements, for this engine: a foreign optimizer is refused and nothing
    moves; an optimizer that stepped through forward() + autograd keeps what it accumulated, re-homed into the engine's
    buffers, and the fused steps go on from it; disagreeing step counters are refused."""
    from tests.test_gpu_engine_handoff import _aliases_engine, _moment_buffers

    m, params, batches, loss = _handoff_model(tmp_path, golden_small)
    eng = m._fused_engine()
    foreign = torch.optim.Adam(params, lr=1e-3)
    held = [t for side in _moment_buffers(eng) for t in side]
    before = [t.detach().clone() for t in params + held]
    assert m.fused_train_step(*batches[0], loss, foreign) is False and m._engine_adam(foreign) is None
    torch.cuda.synchronize()
    for t, was in zip(params + held, before):
        assert torch.equal(t.detach(), was)
    assert not foreign.state
    # one step the other way, then the seam
    opt = ops.Adam(params, lr=1e-3)
    m.fused_loss_and_grad(*batches[0])
    opt.step()
    want = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    assert all(int(opt.state[p]["step"]) == 1 for p in params)
    adam = m._engine_adam(opt)
    assert adam is not None and adam[0] is opt.param_groups[0] and adam[1] == 1
    eng = m._fused_engine()
    for p, (wm, wv) in zip(params, want):
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], wm) and torch.equal(st["exp_avg_sq"], wv) and float(wm.abs().max()) > 0
    assert _aliases_engine(opt, params, eng)
    for b in batches[1:]:
        assert m.fused_train_step(*b, loss, opt) is True and torch.isfinite(loss).all()
    assert m._fused_engine() is eng and all(int(opt.state[p]["step"]) == 3 for p in params)
    assert all(torch.isfinite(p.detach()).all() for p in params) and _aliases_engine(opt, params, eng)
    # one counter runs ahead: no step, no parameter moves
    opt.state[params[-1]]["step"] += 1
    before = [p.detach().clone() for p in params]
    assert m.fused_train_step(*batches[0], loss, opt) is False and m._engine_adam(opt) is None
    torch.cuda.synchronize()
    for p, was in zip(params, before):
        assert torch.equal(p.detach(), was)
    assert [int(opt.state[p]["step"]) for p in params] == [3] * (len(params) - 1) + [4]
