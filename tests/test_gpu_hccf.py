"""HCCF on the GPU: the four kernels of csrc/idg_hyper.hip, ops.hyper_mix, the fused chain (idgrec_amd/hccf.py) and the
plugin (models/HCCF.py) against tests/hccf_ref64.py — the layer, its closed-form gradients and the whole step in plain torch,
which tests/test_hccf_host.py pins to the reference's own float64 numbers.

One tolerance rule throughout (tests/egcf_ref64.py): e_kernel <= band(e_f32) = max(4 e_f32, 8 * 2^-24), where e_f32 is the
distance from float64 of the SAME expressions evaluated in float32 by torch in the same test, both over max |ref64|.  Both
numbers are printed (pytest -s).

  (a) the keep mask: mask_out fed back as `mask` gives the same bits in every kernel that takes one (and the closing call
      on those bits), it is indexed by the global row, another stream id draws another mask, the keep rate over 2.1e6 draws,
      keep = 1.0 keeps everything
  (b) the four raw calls against float64 with explicit masks: nrows 1 .. 129 and one more than 64 rows per resident
      workgroup (512 for latent / expand / close, 256 for the backward: a persistent workgroup takes a second tile and a
      slice holds two), row0 0 / 37, leading dimensions wider than the width, keep 1.0 / 0.5, accumulate off / on, side /
      total present / absent, an all-zero row of E0, NaN in every byte a call must neither read nor write
  (c) two calls give equal bits for L, gW, gHb and Y
  (d) ops.hyper_mix under autograd: at (64, 64) the raw calls' bits; at (32, 16) the torch composition against float64
  (e) HccfEngine: two consecutive steps with different batches at U = 300, I = 250 (the side boundary inside the fifth tile),
      K = 1 and 3, keep 1.0 and 0.5 with injected masks: losses, final, every S_l / Y_l, all gradients, Adam moments and
      parameters against step64 / adam64
  (f) models.HCCF against both goldens with the reference's recorded masks: losses, rating, the three-step trajectory at the
      tolerances tests/test_gpu_bigcf.py group (g) cites; gradients: see test_model_gradients_match_reference_goldens

Measured on an MI355X, e_kernel / e_f32 (and the worst share of the band):
  (b) L, gL, gW 0.05 .. 1.11 (0.28); Y, next, total 0.37 .. 1.92 (0.31); gX, gE0 0.41 .. 1.45 (0.25); gHb 0.29 .. 2.70 (0.68)
  (d) (32, 16): 1.00 (the composition IS the path); hyper_mix(E0, W, E0) within the band
  (e) losses 0.42 .. 2.66 (0.43); final, Y_l 0.42 .. 0.69 (0.17); S_l 0.58 .. 2.76 (0.53); GRAD, gW_u, gW_i 0.22 .. 2.38 (0.60);
      Adam moments <= 2.3 * 2^-24 of their largest entry, parameters <= 1.0 ulp of theirs
  (f) gradients 0.23 .. 1.04 (0.26); rating `def` 0.90 (0.23); keep rate 0.499369 over 2,097,152 draws (allowed 1.74e-3 off)
The file runs in 7 s after the library is loaded (49 cases, the slowest 1.4 s).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import hccf_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
D = H = 64
STREAM = (0x9E3779B97F4A7C15, 11)  # (seed, stream id); the seed does not fit 32 bits
WGS, BWD_WGS = 512, 256            # resident workgroups: latent / expand / close, and the backward (csrc/idg_hyper.hip)
REG, SSL, TEMP, LR = 1e-4, 0.3, 0.1, 1e-3  # configure/HCCF.txt


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rng(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _randn(rng, shape, scale=1.0):
    return dev((rng.standard_normal(shape) * scale).astype(np.float32))


def _check(what, got, ref64, f32):
    e_k, e_f = ref.errors(got, ref64, f32)
    print("  %-70s e_kernel %.2e  e_f32 %.2e  (%.2f of the band)" % (what, e_k, e_f, e_k / ref.band(e_f)))
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- panels indexed by the global row, NaN wherever a call has no business
TAIL = 3


def _panel(clean, row0, ld=D):
    """[row0 + n + TAIL, ld] of NaN with `clean` [n, 64] at rows row0 ..., columns 0 .. 63; returns (whole, view [., 64])."""
    whole = torch.full((row0 + clean.shape[0] + TAIL, ld), NAN, device="cuda")
    whole[row0:row0 + clean.shape[0], :D] = clean
    return whole, whole[:, :D]


def _mask_panel(clean, row0):
    """uint8 [row0 + n + TAIL, 64]: `clean` at rows row0 ..., 1 elsewhere (reading those would keep what must be dropped)."""
    if clean is None:
        return None
    whole = torch.ones((row0 + clean.shape[0] + TAIL, H), dtype=torch.uint8, device="cuda")
    whole[row0:row0 + clean.shape[0]] = clean.to(torch.uint8)
    return whole


def _untouched(whole, row0, n):
    """Everything outside rows row0 .. row0 + n - 1 x columns 0 .. 63 is still NaN."""
    out = torch.isnan(whole)
    return bool(out[:row0].all()) and bool(out[row0 + n:].all()) and bool(out[row0:row0 + n, D:].all())


def _case(n, row0, keep):
    rng = _rng("case", n, row0, keep)
    E0, X, gY, gHb = _randn(rng, (n, D), 0.3), _randn(rng, (n, D), 0.5), _randn(rng, (n, D)), _randn(rng, (n, H))
    W = _randn(rng, (D, H), 0.2)
    if n > 2:
        E0[n // 2] = 0  # an all-zero row
    mask = dev(rng.random((n, H)) < keep) if keep < 1.0 else None
    return E0, W, X, gY, gHb, mask, rng


# ============================================================================================================ (a) the mask
def test_keep_mask_is_a_function_of_the_global_row_and_the_stream(ops):
    n, row0, keep = 32768, 37, 0.5  # 32768 x 64 = 2,097,152 draws
    rng = _rng("mask")
    E0, X, gY = _randn(rng, (row0 + n, D), 0.3), _randn(rng, (row0 + n, D), 0.5), _randn(rng, (row0 + n, D))
    W = _randn(rng, (D, H), 0.2)
    seed, sid = STREAM
    gen = dict(keep=keep, seed=seed, stream_id=sid)
    m0 = torch.full((row0 + n, H), 7, dtype=torch.uint8, device="cuda")
    L0 = ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), row0=0, mask_out=m0, **gen)
    assert bool(((m0 == 0) | (m0 == 1)).all())
    # indexing is by the global row: rows 37 .. of a call that starts at row 0 = a call that starts at row 37
    m37 = torch.full((row0 + n, H), 7, dtype=torch.uint8, device="cuda")
    L37 = ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), row0=row0, nrows=n, mask_out=m37, **gen)
    assert bool((m37[:row0] == 7).all()) and torch.equal(m37[row0:], m0[row0:])
    # the keep rate over N draws: within 5 sigma + the 16-bit threshold of keep_of_bits
    N = n * H
    rate = float(m37[row0:].double().mean())
    bound = 5 * np.sqrt(keep * (1 - keep) / N) + 2.0 ** -16
    print("  keep rate %.6f over %d draws (|rate - keep| = %.2e, allowed %.2e)" % (rate, N, abs(rate - keep), bound))
    assert N >= 2_000_000 and abs(rate - keep) <= bound
    # another stream id draws another mask
    m_other = torch.zeros_like(m0)
    ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), row0=0, mask_out=m_other, keep=keep, seed=seed, stream_id=sid + 1)
    agree = float((m_other == m0).double().mean())
    assert abs(agree - 0.5) < 0.01 and abs(float(m_other.double().mean()) - keep) <= bound
    # mask_out fed back as `mask` gives the same bits in every kernel that takes one
    fed = dict(keep=keep, mask=m0)
    assert torch.equal(_bits(ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), row0=0, **fed)), _bits(L0))
    assert torch.equal(_bits(ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), row0=row0, nrows=n, **fed)), _bits(L37))
    Yg, Yf = (ops.hyper_expand_raw(E0, W, L0, torch.empty_like(X), row0=0, **kw) for kw in (gen, fed))
    assert torch.equal(_bits(Yg), _bits(Yf))
    gL = ops.hyper_latent_raw(E0, W, gY, torch.empty(H, D, device="cuda"), row0=0, **gen)
    outs = []
    for kw in (gen, fed):
        gX, gHb = torch.zeros_like(X), torch.empty(row0 + n, H, device="cuda")
        ops.hyper_bwd_raw(E0, W, X, gY, L0, gL, gX, gHb, row0=0, **kw)
        gE0, gW = torch.zeros_like(E0), torch.empty(D, H, device="cuda")
        ops.hyper_close_raw(E0, W, gHb, gE0, gW, row0=0)
        outs.append((gX, gHb, gE0, gW))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    assert bool((outs[0][1][m0 == 0] == 0).all())  # a dropped element passes no gradient
    # keep = 1.0 keeps everything
    m1 = torch.zeros_like(m0)
    ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), row0=0, mask_out=m1, keep=1.0, seed=seed, stream_id=sid)
    assert bool((m1 == 1).all())


# ============================================================================================================ (b) the raw calls
LAYER_N = [1, 63, 64, 65, 129, 64 * BWD_WGS + 1, 64 * WGS + 1]


@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("row0", [0, 37])
@pytest.mark.parametrize("n", LAYER_N)
def test_hyper_kernels_vs_float64(ops, n, row0, keep):
    E0, W, X, gY, gHb_in, mask, rng = _case(n, row0, keep)
    wide = row0 == 37  # the second row0 also takes leading dimensions wider than the width
    ld = (lambda k: D + 4 * k) if wide else (lambda k: D)
    mp = _mask_panel(mask, row0)
    kw = dict(row0=row0, nrows=n, keep=keep, mask=mp)
    r64 = {dt: ref.layer64(E0, W, X, mask, keep, dtype=dt) for dt in (F64, F32)}  # (Y, L, H)
    # ---- latent
    E0w, E0p = _panel(E0, row0, ld(1))
    Xw, Xp = _panel(X, row0, ld(2))
    L = ops.hyper_latent_raw(E0p, W, Xp, torch.full((H, D), NAN, device="cuda"), **kw)
    tag = "n=%d row0=%d keep=%g " % (n, row0, keep)
    _check(tag + "L", L, r64[F64][1], r64[F32][1])
    # ---- expand: Y alone, then with side / next / total; L as the float64 statement's, rounded
    L_in = r64[F64][1].to(F32)
    y = {dt: ref.hyper64(E0, W, mask, keep, dt) @ L_in.to(dt) for dt in (F64, F32)}
    side, tot0 = _randn(rng, (n, D)), _randn(rng, (n, D))
    Yw, Yp = _panel(torch.full((n, D), NAN, device="cuda"), row0, ld(3))
    ops.hyper_expand_raw(E0p, W, L_in, Yp, **kw)
    _check(tag + "Y", Yw[row0:row0 + n, :D], y[F64], y[F32])
    assert _untouched(Yw, row0, n)
    Y_alone = Yw[row0:row0 + n, :D].clone()
    Sw, Sp = _panel(side, row0, ld(1))
    Nw, Np = _panel(torch.full((n, D), NAN, device="cuda"), row0, ld(2))
    Tw, Tp = _panel(tot0, row0, ld(0))
    Yw.fill_(NAN)
    ops.hyper_expand_raw(E0p, W, L_in, Yp, side=Sp, next=Np, total=Tp, **kw)
    assert torch.equal(_bits(Yw[row0:row0 + n, :D]), _bits(Y_alone))
    _check(tag + "next", Nw[row0:row0 + n, :D], side.double() + y[F64], side + y[F32])
    _check(tag + "total", Tw[row0:row0 + n, :D], tot0.double() + side.double() + y[F64], tot0 + (side + y[F32]))
    assert _untouched(Yw, row0, n) and _untouched(Nw, row0, n) and _untouched(Tw, row0, n)
    Tw[row0:row0 + n, :D] = tot0
    ops.hyper_expand_raw(E0p, W, L_in, Yp, total=Tp, **kw)  # total without side: += Y
    _check(tag + "total (no side)", Tw[row0:row0 + n, :D], tot0.double() + y[F64], tot0 + y[F32])
    # ---- backward: gL from the latent call on gY, then gX / gHb, accumulate off and on
    GYw, GYp = _panel(gY, row0, ld(2))
    gL = ops.hyper_latent_raw(E0p, W, GYp, torch.full((H, D), NAN, device="cuda"), **kw)
    g = {dt: ref.layer_grads64(E0, W, X, gY, mask, keep, dtype=dt) for dt in (F64, F32)}  # (gL, H gL, M o gH / keep)
    _check(tag + "gL", gL, g[F64][0], g[F32][0])
    gL_in = g[F64][0].to(F32)
    b = {}
    for dt in (F64, F32):
        Hm, Lc, gLc = ref.hyper64(E0, W, mask, keep, dt), L_in.to(dt), gL_in.to(dt)
        gH = gY.to(dt) @ Lc.t() + X.to(dt) @ gLc.t()
        scale = 1.0 if keep >= 1.0 else 1.0 / keep
        b[dt] = (Hm @ gLc, gH * scale if mask is None else gH * (mask.to(dt) * scale))
    gx0 = _randn(rng, (n, D))
    for acc in (False, True):
        GXw, GXp = _panel(gx0, row0, ld(1))
        GHw, GHp = _panel(gHb_in if acc else torch.full((n, H), NAN, device="cuda"), row0, ld(3))
        ops.hyper_bwd_raw(E0p, W, Xp, GYp, L_in, gL_in, GXp, GHp, accumulate=acc, **kw)
        what = tag + ("accumulate " if acc else "store ")
        _check(what + "gX", GXw[row0:row0 + n, :D], gx0.double() + b[F64][0], gx0 + b[F32][0])
        _check(what + "gHb", GHw[row0:row0 + n, :H], (gHb_in.double() if acc else 0) + b[F64][1], (gHb_in if acc else 0) + b[F32][1])
        assert _untouched(GXw, row0, n) and _untouched(GHw, row0, n)
        if mask is not None:
            assert bool(((GHw[row0:row0 + n, :H] - (gHb_in if acc else 0))[~mask] == 0).all())
    # ---- close
    GHw, GHp = _panel(gHb_in, row0, ld(2))
    ge0 = _randn(rng, (n, D))
    GEw, GEp = _panel(ge0, row0, ld(1))
    gW = torch.full((D, H), NAN, device="cuda")
    ops.hyper_close_raw(E0p, W, GHp, GEp, gW, row0=row0, nrows=n)
    c = {dt: ref.close64(E0, W, gHb_in, dtype=dt) for dt in (F64, F32)}
    _check(tag + "gE0", GEw[row0:row0 + n, :D], ge0.double() + c[F64][0], ge0 + c[F32][0])
    _check(tag + "gW", gW, c[F64][1], c[F32][1])
    assert _untouched(GEw, row0, n)
    # the all-zero row of E0: H is zero there, whatever the mask
    assert n <= 2 or bool((Y_alone[n // 2] == 0).all())
    # no input was written
    for whole, clean in ((E0w, E0), (Xw, X), (GYw, gY), (GHw, gHb_in), (Sw, side)):
        assert torch.equal(_bits(whole[row0:row0 + n, :D]), _bits(clean)) and _untouched(whole, row0, n)
    if mp is not None:
        assert torch.equal(mp[row0:row0 + n], mask.to(torch.uint8)) and bool((mp[:row0] == 1).all()) and bool((mp[row0 + n:] == 1).all())


# ============================================================================================================ (c) equal bits
@pytest.mark.parametrize("n", [129, 64 * WGS + 1])
def test_two_runs_give_equal_bits(ops, n):
    E0, W, X, gY, gHb_in, mask, _ = _case(n, 0, 0.5)
    runs = []
    for _ in range(2):
        kw = dict(keep=0.5, mask=mask)
        L = ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), **kw)
        Y = ops.hyper_expand_raw(E0, W, L, torch.empty_like(X), **kw)
        gL = ops.hyper_latent_raw(E0, W, gY, torch.empty(H, D, device="cuda"), **kw)
        gX, gHb = torch.zeros_like(X), torch.empty(n, H, device="cuda")
        ops.hyper_bwd_raw(E0, W, X, gY, L, gL, gX, gHb, **kw)
        gE0, gW = torch.zeros_like(E0), torch.empty(D, H, device="cuda")
        ops.hyper_close_raw(E0, W, gHb, gE0, gW)
        runs.append((L, Y, gL, gX, gHb, gE0, gW))
    for name, a, b in zip(("L", "Y", "gL", "gX", "gHb", "gE0", "gW"), *runs):
        assert torch.isfinite(a).all() and torch.equal(_bits(a), _bits(b)), name


# ============================================================================================================ (d) hyper_mix
def test_autograd_at_64_64_is_the_raw_calls_bit_for_bit(ops):
    n, row0 = 200, 37
    E0, W, X, gY, _, mask, _ = _case(n, row0, 0.5)
    seed, sid = STREAM
    for kw_mix, kw_raw in ((dict(mask=mask), dict(mask=mask)), (dict(stream=STREAM), dict(seed=seed, stream_id=sid))):
        e, w, x = (t.clone().requires_grad_(True) for t in (E0, W, X))
        Y = ops.hyper_mix(e, w, x, row0=row0, keep=0.5, **kw_mix)
        Y.backward(gY)
        raw = dict(row0=row0, base_row=row0, keep=0.5, **kw_raw)
        L = ops.hyper_latent_raw(E0, W, X, torch.empty(H, D, device="cuda"), **raw)
        Yr = ops.hyper_expand_raw(E0, W, L, torch.empty_like(X), **raw)
        gL = ops.hyper_latent_raw(E0, W, gY, torch.empty(H, D, device="cuda"), **raw)
        gX, gHb = torch.zeros_like(X), torch.empty(n, H, device="cuda")
        ops.hyper_bwd_raw(E0, W, X, gY, L, gL, gX, gHb, **raw)
        gE0, gW = torch.zeros_like(E0), torch.empty(D, H, device="cuda")
        ops.hyper_close_raw(E0, W, gHb, gE0, gW, row0=row0, base_row=row0)
        for name, a, b in (("Y", Y.detach(), Yr), ("gE0", e.grad, gE0), ("gW", w.grad, gW), ("gX", x.grad, gX)):
            assert torch.equal(_bits(a), _bits(b)), name
    # E0 and X the SAME tensor (layer 0): the two gradients are added
    e = E0.clone().requires_grad_(True)
    ops.hyper_mix(e, W, e, row0=row0, keep=0.5, mask=mask).backward(gY)
    t64 = E0.double().requires_grad_(True)
    (want,) = torch.autograd.grad((ref.layer64(t64, W, t64, mask, 0.5)[0] * gY.double()).sum(), t64)
    t32 = E0.clone().requires_grad_(True)
    (f32,) = torch.autograd.grad((ref.layer64(t32, W, t32, mask, 0.5, dtype=F32)[0] * gY).sum(), t32)
    _check("hyper_mix(E0, W, E0) d E0", e.grad, want, f32)


def test_autograd_at_32_16_vs_float64(ops):
    n, d, h = 150, 32, 16
    rng = _rng("32x16")
    E0, X, gY, W = _randn(rng, (n, d), 0.3), _randn(rng, (n, d), 0.5), _randn(rng, (n, d)), _randn(rng, (d, h), 0.3)
    mask = dev(rng.random((n, h)) < 0.5)
    e, w, x = (t.clone().requires_grad_(True) for t in (E0, W, X))
    Y = ops.hyper_mix(e, w, x, row0=5, keep=0.5, mask=mask)
    Y.backward(gY)
    outs = {}
    for dt in (F64, F32):
        leaves = [t.to(dt).requires_grad_(True) for t in (E0, W, X)]
        y = ref.layer64(*leaves, mask, 0.5, dtype=dt)[0]
        outs[dt] = (y.detach(),) + torch.autograd.grad((y * gY.to(dt)).sum(), leaves)
    for name, got, a, b in zip(("Y", "gE0", "gW", "gX"), (Y.detach(), e.grad, w.grad, x.grad), outs[F64], outs[F32]):
        _check("(32, 16) " + name, got, a, b)
    # without a mask at keep < 1 the composed path draws one with torch: about half is dropped
    Yd = ops.hyper_mix(E0, W, X, keep=0.5)
    assert torch.isfinite(Yd).all() and not torch.equal(Yd, ops.hyper_mix(E0, W, X, keep=1.0))


# ================================================================================================================ (e) the engine
ENGINE = [(1, 1.0), (3, 1.0), (1, 0.5), (3, 0.5)]
_engine_runs = {}
_graphs = {}


@pytest.fixture(scope="module")
def golden_hccf():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "hccf_small.npz"), allow_pickle=False))
    g.update(np.load(os.path.join(ROOT, "tests", "golden", "hccf_small_drop.npz"), allow_pickle=False))
    return g


def _graph(ops, golden_small):
    if "g" not in _graphs:
        g = golden_small
        n = int(g["num_users"]) + int(g["num_items"])
        _graphs["g"] = (ops.Graph(g["adj_indptr"], g["adj_indices"], g["adj_data"], n, n),
                        ref.dense_operator(g["adj_indptr"], g["adj_indices"], g["adj_data"], (n, n), device="cuda"))
    return _graphs["g"]


def _engine_run(ops, golden_small, golden_hccf, K, keep):
    """Two training steps — the B = 96 batch with duplicate users and items, then a 256-row one — every step next to step64 in
    float64 and float32 FROM THE ENGINE'S OWN PARAMETERS read back before the step, with the step's masks (injected at
    keep < 1).  U = 300: the user / item boundary falls inside the fifth 64-row tile."""
    if (K, keep) in _engine_runs:
        return _engine_runs[(K, keep)]
    from idgrec_amd.hccf import HccfEngine

    G, A64 = _graph(ops, golden_small)
    U, I = int(golden_small["num_users"]), int(golden_small["num_items"])
    n = U + I
    rng = _rng("engine", K, keep)
    xav = lambda r, c: dev(rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32))  # noqa: E731
    P0 = torch.cat([xav(U, D), xav(I, D)])
    W0 = (xav(D, H), xav(D, H))
    batches = [tuple(dev(golden_hccf["batch"][:, c]) for c in range(3)),
               tuple(dev(golden_hccf["traj_batches"][256:512, c]) for c in range(3))]  # ([:256] contains the B = 96 batch)
    masks = [dev(rng.random((K, n, H)) < keep).to(torch.uint8) if keep < 1.0 else None for _ in batches]
    eng = HccfEngine(G, U, I, P0.clone(), W0, K, keep=keep, reg_lambda=REG, ssl_lambda=SSL, temperature=TEMP, lr=LR, store_grad=True)
    SW0 = eng.SW.clone()
    steps = []
    for s, (users, pos, neg) in enumerate(batches):
        P_before, (Wu, Wi) = eng.P.clone(), (v.clone() for v in eng.hyper_views())
        loss = eng.train_step(users, pos, neg, masks=masks[s]).clone()
        st = dict(loss=loss, GRAD=eng.GRAD.clone(), SG=eng.SG.clone(), P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(),
                  SW=eng.SW.clone(), SM=eng.SM.clone(), SV=eng.SV.clone(), final=eng.FINAL.clone(),
                  S=[t.clone() for t in eng.S], Y=[t.clone() for t in eng.Y])
        mb = None if masks[s] is None else masks[s].bool()
        for name, dtype in (("64", F64), ("32", F32)):
            losses, (gE0, gWu, gWi), fin, S_, Y_ = ref.step64(A64, P_before, Wu, Wi, users, pos, neg, K, mb, keep, REG, SSL, TEMP, U, dtype=dtype)
            st["loss" + name], st["GRAD" + name], st["final" + name], st["S" + name], st["Y" + name] = losses, gE0, fin, S_, Y_
            st["SG" + name] = torch.cat([gWu.reshape(-1), gWi.reshape(-1)])
        steps.append(st)
    assert eng.step_count == 2
    run = dict(P0=P0, SW0=SW0, steps=steps)
    torch.cuda.synchronize()
    _engine_runs[(K, keep)] = run
    return run


@pytest.mark.parametrize("K,keep", ENGINE)
def test_engine_two_steps_vs_float64(ops, golden_small, golden_hccf, K, keep):
    """The second step's batch names other rows than the first's: rows of step 1 leaking into step 2 — through gFinal
    (cleared and stored per step), through the regulariser's panel (read at the batch's rows only), through gHb (stored by the
    first layer of every backward) — would show in its gradients."""
    run = _engine_run(ops, golden_small, golden_hccf, K, keep)
    per = D * H
    for s, st in enumerate(run["steps"], 1):
        tag = "engine K=%d keep=%g step %d" % (K, keep, s)
        assert torch.isfinite(st["loss"]).all() and torch.isfinite(st["GRAD"]).all() and torch.isfinite(st["SG"]).all()
        for k, name in enumerate(("bpr", "reg", "ssl")):
            _check("%s loss %s" % (tag, name), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " final", st["final"], st["final64"], st["final32"])
        for l in range(K):
            _check("%s S_%d" % (tag, l), st["S"][l], st["S64"][l], st["S32"][l])
            _check("%s Y_%d" % (tag, l), st["Y"][l], st["Y64"][l], st["Y32"][l])
        _check(tag + " GRAD", st["GRAD"], st["GRAD64"], st["GRAD32"])
        for i, name in enumerate(("gW_u", "gW_i")):
            _check("%s %s" % (tag, name), st["SG"][i * per:(i + 1) * per], st["SG64"][i * per:(i + 1) * per], st["SG32"][i * per:(i + 1) * per])
    rows = [set(np.concatenate([b[:, 0], 300 + b[:, 1], 300 + b[:, 2]]).tolist())
            for b in (golden_hccf["batch"], golden_hccf["traj_batches"][256:512])]
    assert len(rows[0] - rows[1]) > 20


@pytest.mark.parametrize("K,keep", ENGINE)
def test_engine_adam_state_after_each_step(ops, golden_small, golden_hccf, K, keep):
    """tests/test_gpu_bigcf.py::test_engine_adam_state_after_each_step: on the embedding panel and on the flat buffer
    [W_u | W_i] (one launch each): exp_avg, exp_avg_sq within 4 * 2^-24 of their largest entry, the parameters within 4 ulp of
    their largest entry, against the float64 recurrence fed the engine's own two gradients from the float32 initial values."""
    run = _engine_run(ops, golden_small, golden_hccf, K, keep)
    for what, W0, gk, wk, mk, vk in (("panel", run["P0"], "GRAD", "P", "M", "V"), ("hypers", run["SW0"], "SG", "SW", "SM", "SV")):
        want = ref.adam64(W0, [st[gk] for st in run["steps"]], lr=LR)
        for s, (st, (W, M, V)) in enumerate(zip(run["steps"], want), 1):
            for name, got, w in (("exp_avg", st[mk], M), ("exp_avg_sq", st[vk], V)):
                e = float((got.double() - w).abs().max() / w.abs().max())
                print("  K=%d keep=%g %s step %d %s: %.2f * 2^-24 of max" % (K, keep, what, s, name, e * 2.0 ** 24))
                assert e <= 4 * 2.0 ** -24, (what, name, s, e)
            wmax = float(W.abs().max())
            ulp = float(np.spacing(np.float32(wmax)))
            e = float((st[wk].double() - W).abs().max())
            print("  K=%d keep=%g %s step %d parameters: %.2f ulp of max |W| = %.3f" % (K, keep, what, s, e / ulp, wmax))
            assert e <= 4 * ulp, (what, s, e / ulp)
        assert not torch.equal(run["steps"][0][wk], run["steps"][1][wk])


# ================================================================================================================ (f) the plugin
PARAMS = ("user_embedding", "item_embedding", "user_hyper_emb", "item_hyper_emb")
SETTINGS = [("def", 1.0, 3), ("drop", 0.5, 2)]
# the gradients held by the band rule (see test_model_gradients_match_reference_goldens); the others by the cited tolerance
BAND_RULE = {("def", "user_embedding"), ("def", "item_embedding"), ("def", "user_hyper_emb"),
             ("drop", "user_embedding"), ("drop", "item_embedding"), ("drop", "user_hyper_emb"), ("drop", "item_hyper_emb")}


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "HCCF.txt"), "HCCF")
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


def _model(tmp_path, golden_small, keep, K, **kw):
    import utility.utility_function.tools as tools
    from models.HCCF import HCCF

    cfg = _cfg(GCN_layer=K, keeprate=keep, **kw)
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = HCCF(cfg, data, torch.device("cuda")).to("cuda")
    return cfg, m, {p: getattr(m, p).weight for p in PARAMS}


def _recorded(g, tag, name):
    key = "%s_masks_%s" % (tag, name)
    return ref.unpack_masks(g[key]).to(torch.uint8).cuda().contiguous() if key in g else None


@pytest.mark.parametrize("tag,keep,K", SETTINGS)
def test_model_losses_and_rating_match_reference_goldens(ops, tag, keep, K, tmp_path, golden_small, golden_hccf):
    """Losses and rating at the tolerances of tests/test_gpu_bigcf.py::test_model_losses_and_rating_match_reference_goldens
    (losses rtol 1e-4; rating rtol 1e-4 with atol 1e-5); the reference's recorded masks are injected.  The constructor replays
    the reference's order of draws: a torch seed gives the reference's initial tables.

    The rating of `def` is held by the band rule instead of the cited tolerance: without dropout three layers of H (H^T X) grow
    final to entries of 53 and the scores to 5.3e3, where one float32 rounding of a score is 5e-4 — the float32 COMPOSITION of
    the reference's expressions (tests/hccf_ref64.py in float32, on the CPU) has 5 of the 8,000 ratings outside rtol 1e-4 /
    atol 1e-5, the worst at 1.38 of it.  The tolerance is not loosened: e <= max(4 e_f32, 8 * 2^-24) over max |float64| with
    e_f32 the float32 composition's distance in this very test; `drop` (scores to 238, composition at 0.24) keeps the cited
    tolerance.  Both shares are printed."""
    g = golden_hccf
    cfg, m, prm = _model(tmp_path, golden_small, keep, K)
    assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
    for p in PARAMS:  # same torch RNG order as the reference's constructor
        assert np.array_equal(prm[p].detach().cpu().numpy(), g["init_" + p]), p
    b = torch.from_numpy(g["batch"]).cuda()
    fwd = _recorded(g, tag, "fwd")
    final, gnn, hyper = m.aggregate(masks=fwd)
    assert tuple(final.shape) == (550, 64) and len(gnn) == len(hyper) == K
    m.mask_source = lambda: fwd
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 3
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-4)
    m.eval()
    users = torch.from_numpy(g["rating_users"]).cuda()
    rmask = _recorded(g, tag, "rating")
    m.mask_source = None if rmask is None else (lambda: rmask)
    _, A64 = _graph(ops, golden_small)
    E0 = torch.cat([dev(g["init_user_embedding"]), dev(g["init_item_embedding"])])
    Wu, Wi = dev(g["init_user_hyper_emb"]), dev(g["init_item_hyper_emb"])
    r = {}
    for dt in (F64, F32):
        fin = ref.aggregate64(A64, E0, Wu, Wi, 300, K, None if rmask is None else rmask.bool(), keep, dtype=dt)[0]
        r[dt] = torch.sigmoid(fin[users] @ fin[300:].t())
    want = g[tag + "_rating"]
    assert float(np.abs(r[F64].cpu().numpy() - want).max()) <= 2.0 ** -23  # the float64 statement is the golden
    tol = 1e-5 + 1e-4 * np.abs(want)
    for got in (m.get_rating_for_test(users, masks=rmask), m.get_rating_for_test(users)):
        share, share32 = np.abs(got.cpu().numpy() - want) / tol, np.abs(r[F32].cpu().numpy() - want) / tol
        print("rating %s: worst %.2f of rtol 1e-4 / atol 1e-5 (the float32 composition: %.2f)" % (tag, share.max(), share32.max()))
        if tag == "def":
            _check("rating def", got, r[F64], r[F32])
        else:
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-5)
    m.mask_source = None
    if keep < 1.0:
        # evaluation draws its own masks otherwise: one draw per pass (cached while the weights are frozen), another the next
        m.train()
        m.eval()
        r1, r2 = m.get_rating_for_test(users), m.get_rating_for_test(users)
        assert torch.equal(r1, r2) and torch.isfinite(r1).all() and not torch.equal(r1.cpu(), torch.from_numpy(g[tag + "_rating"]))
        m.train()
        m.eval()
        assert not torch.equal(m.get_rating_for_test(users), r1)
    assert m.topk_for_test(users, 10).shape == (32, 10)


@pytest.mark.parametrize("tag,keep,K", SETTINGS)
def test_model_gradients_match_reference_goldens(ops, tag, keep, K, tmp_path, golden_small, golden_hccf):
    """Every .grad of forward() + backward() against the reference's (float64, rounded to float32).

    tests/test_gpu_bigcf.py group (g) cites rtol 1e-3 with atol 1e-8 on the two tables and 1e-7 on the two matrices.  On this
    fixture the float32 COMPOSITION of the reference's own expressions (tests/hccf_ref64.py in float32, on the CPU) misses
    that tolerance itself: HCCF's gradients are dense — every row of both tables, through H^T X — with a largest entry of
    1.7 (`def`) / 6.1 (`drop`) next to elements of 1e-7, and an element-wise relative tolerance asks of those elements what
    float32 sums of that size cannot give.  Worst element as a share of the tolerance, float32 composition: `def` 13.0 / 7.1 /
    1.43 / 0.95, `drop` 7.2 / 12.0 / 4.5 / 2.4 (user_embedding / item_embedding / user_hyper_emb / item_hyper_emb).  The
    tolerance is not loosened: the seven tensors whose float32 composition exceeds it are held by the band rule instead,
    e <= max(4 e_f32, 8 * 2^-24) over max |float64|, with e_f32 the float32 composition's distance in this very test;
    `def` item_hyper_emb keeps the cited tolerance (measured on an MI355X: 0.9986 of it at the worst element, the float32
    composition 0.9755 there; the kernels and every operator of forward() are deterministic, so that figure repeats).  For each gradient the worst element's share of the cited tolerance is
    printed next to the float32 composition's own share."""
    g = golden_hccf
    fwd = _recorded(g, tag, "fwd")
    cfg, m, prm = _model(tmp_path, golden_small, keep, K)
    b = torch.from_numpy(g["batch"]).cuda()
    m.zero_grad()
    ll = m(b[:, 0], b[:, 1], b[:, 2], masks=fwd)
    sum(ll).backward()
    _, A64 = _graph(ops, golden_small)
    E0 = torch.cat([dev(g["init_user_embedding"]), dev(g["init_item_embedding"])])
    Wu, Wi = dev(g["init_user_hyper_emb"]), dev(g["init_item_hyper_emb"])
    mb = None if fwd is None else fwd.bool()
    r = {dt: ref.step64(A64, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], K, mb, keep, REG, SSL, TEMP, 300, dtype=dt)[1] for dt in (F64, F32)}
    split = lambda t: dict(zip(PARAMS, (t[0][:300], t[0][300:], t[1], t[2])))  # noqa: E731
    g64, g32 = split(r[F64]), split(r[F32])
    failed = []
    for p, atol in zip(PARAMS, (1e-8, 1e-8, 1e-7, 1e-7)):
        mine, want = prm[p].grad.cpu().numpy(), g["%s_grad_%s" % (tag, p)]
        tol = atol + 1e-3 * np.abs(want)
        share, share32 = np.abs(mine - want) / tol, np.abs(g32[p].cpu().numpy() - want) / tol
        e_k, e_f = ref.errors(prm[p].grad, g64[p], g32[p])
        rule = "band" if (tag, p) in BAND_RULE else "cited tolerance"
        print("grad %s %s [%s]: worst %.4f of rtol 1e-3 / atol %g (the float32 composition: %.4f); e_kernel %.2e, e_f32 %.2e (%.2f of the "
              "band); max |g| %.3g" % (tag, p, rule, share.max(), atol, share32.max(), e_k, e_f, e_k / ref.band(e_f), np.abs(want).max()))
        ok = e_k <= ref.band(e_f) if (tag, p) in BAND_RULE else bool((share <= 1).all())
        if not ok:
            failed.append(p)
        # the float64 statement is the golden (tests/test_hccf_host.py): the band's reference is the reference's number
        assert float(np.abs(g64[p].cpu().numpy() - want).max()) <= 2.0 ** -23 * float(np.abs(want).max())
    assert not failed, failed


@pytest.mark.parametrize("tag,keep,K", SETTINGS)
def test_model_fused_steps_match_reference_trajectory(ops, tag, keep, K, tmp_path, golden_small, golden_hccf):
    """Three fused steps against the reference's own Adam trajectory, at the tolerances of
    tests/test_gpu_bigcf.py::test_model_fused_steps_match_reference_trajectory; the recorded masks of every step are injected."""
    g = golden_hccf
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    tm = _recorded(g, tag, "traj")
    cfg, m, prm = _model(tmp_path, golden_small, keep, K)
    assert m.fused_step_available()
    if tm is not None:
        seq = iter(tm[i].contiguous() for i in range(3))
        m.mask_source = lambda: next(seq)
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 3), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    for p in PARAMS:
        mine, want = prm[p].detach().cpu().numpy(), g["%s_traj_%s" % (tag, p)]
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("trajectory %s: off %.3g, max %.3g" % (p, off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, (p, off.mean())
        assert np.abs(mine - want).max() < 1e-4, (p, np.abs(mine - want).max())
    assert all(int(opt.state[q]["step"]) == 3 for q in m.parameters())


def test_model_at_other_widths_trains_through_autograd(ops, tmp_path, golden_small):
    """hyper_size = 16: no kernel at that width and no fused step; the differentiable path gives finite losses and a gradient
    for every parameter."""
    rng = _rng("batch")
    b = [dev(rng.integers(0, hi, 128).astype(np.int64)) for hi in (300, 250, 250)]
    cfg, m, prm = _model(tmp_path, golden_small, 0.5, 2, hyper_size=16)
    assert not m.fused_step_available()
    m.train()
    ll = m(*b)
    sum(ll).backward()
    assert len(ll) == 3 and all(torch.isfinite(x).all() for x in ll)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name


def test_invalid_arguments_are_refused_without_device_work(ops):
    """IDG_E_INVALID from the library for real device tensors too: the outputs stay as they were."""
    from idgrec_amd import native

    n = 10
    E0, X = torch.zeros(n, D, device="cuda"), torch.zeros(n, D, device="cuda")
    L = torch.full((H, D), 5.0, device="cuda")
    Y = torch.full((n, D), 5.0, device="cuda")
    for W in (torch.zeros(32, 16, device="cuda"), torch.zeros(64, 128, device="cuda")):
        with pytest.raises(native.IdgError, match=r"\(64, 64\) only"):
            ops.hyper_latent_raw(E0, W, X, L)
    W = torch.zeros(D, H, device="cuda")
    for call, word in ((lambda: ops.hyper_expand_raw(E0, W, L, E0), "overlaps an input"),
                       (lambda: ops.hyper_latent_raw(E0, W, X, L, keep=0.0), "not positive"),
                       (lambda: ops.hyper_latent_raw(E0, W, X, L, row0=-1, nrows=5), "bad sizes"),
                       (lambda: ops.hyper_expand_raw(E0, W, L, Y, side=X), "come together"),
                       (lambda: ops.hyper_bwd_raw(E0, W, X, X, L, L, Y, Y[:, :]), "two outputs overlap"),
                       (lambda: ops.hyper_close_raw(E0, W, X, E0, L), "overlaps an input")):
        with pytest.raises(native.IdgError, match=word):
            call()
    torch.cuda.synchronize()
    assert bool((L == 5.0).all()) and bool((Y == 5.0).all()) and bool((E0 == 0).all())
