"""BIGCF's intent kernels (idgrec_amd/csrc/idg_intent.hip), their differentiable wrapper (ops.intent_mix), the self-contrast
InfoNCE, and the plugin (models/BIGCF.py) on the device.  The reference statement is tests/bigcf_ref64.py, pinned to the
reference's own numbers by tests/test_bigcf_host.py.

  (a) the noise: noise_out is the Z that noise = NULL used (forward and backward fed noise_out give the same bits), the
      global-row indexing, other streams / rows draw other numbers, mean and variance over 2.1 M draws;
  (b) idg_intent_fwd_f32 / idg_intent_bwd_f32 against float64 with explicit noise: 1, 63, 64, 65, 129 and 64 * 512 + 1 rows,
      row0 = 0 / 37, no bitmap / a 5 % bitmap / first and last row only, gT_in present / absent, leading dimensions wider
      than d, NaN in every byte the call must not read or write, logits scaled to max |S| = 100, one all-zero row of X;
  (c) run to run: two calls give equal bits, gW included;
  (d) ops.intent_mix under autograd: the raw calls' bits at (64, 128), the torch composition at (32, 16);
  (e) infonce_pair with view1 is view2, dedup = False and duplicate ids against float64: loss and summed gradient;
  (f) BigcfEngine, two consecutive steps with different batches at U = 300, I = 250 (the user / item boundary inside a
      64-row tile): losses, F, T, every gradient, Adam state, parameters;
  (g) models.BIGCF against the reference's goldens (tests/golden/bigcf_small.npz) with the recorded noise injected.

One tolerance rule throughout (egcf_ref64.errors / band): with scale = max |ref64| of the tensor compared,
    e_kernel = max |kernel - ref64| / scale   <=   max(4 e_f32, 8 * 2^-24),   e_f32 = max |float32 composition - ref64| / scale
where the float32 composition is bigcf_ref64's same expressions in float32, run in the same test; both numbers are printed
(pytest -s).  Kernel and reference share Z and W in float32.

(f)'s Adam state follows tests/test_gpu_gccf.py::test_engine_adam_state_after_each_step; (g) uses the tolerances of
tests/test_gpu_models.py::test_ngcf_vs_reference (losses, gradients, rating) and of
tests/test_gpu_lgcnpp.py::test_model_matches_reference_goldens (the three-step trajectory).

Measured on an MI355X (35 tests, 7.2 s for the whole file once the library is loaded), e_kernel / e_f32 over all comparisons
of a group, worst e_kernel / band:
  (a) exact: F, T, gX, gW with generated noise equal the calls fed noise_out bit for bit; 2,101,312 draws: mean 3.9e-4
      (bound 3.4e-3), var - 1 = -3.0e-4 (bound 4.9e-3)
  (b) 2.5e-8 .. 5.6e-5 / 2.5e-8 .. 5.6e-5 (0.59: n = 63, row0 = 37, the 5 % bitmap, gT at half of the rows, gX), 288 comparisons;
      every other bit of the panels is the NaN it was.  With ONE accumulation chain per product the kernels sat at ~1.4 e_f32
      throughout and one comparison (n = 129, rows 0 and n - 1, gX) reached 1.02 of the band: the products now run as two
      chains (csrc/idg_intent.hip)
  (c), (d) at (64, 128): equal bits; (d) at (32, 16): 1.9e-7 .. 3.8e-7 / 1.9e-7 .. 4.3e-7 (0.25)
  (e) 1.5e-8 .. 4.7e-6 / 2.7e-8 .. 4.3e-6 (0.36: B = 96, added into a panel)
  (f) 5.3e-9 .. 5.7e-6 / 1.2e-8 .. 2.2e-5 (0.37: K = 2, step 1, F), 48 comparisons; Adam moments at most 3.01 * 2^-24 of their
      largest entry, parameters at most 1.00 ulp of theirs
  (g) losses within 2e-7 of the reference's (relative); trajectory: at most 7.3e-4 of a tensor's elements outside rtol 1e-4 /
      atol 1e-6 (user_intent, GCN_layer = 2), at most 3.0e-5 off.  Gradients: at most 0.89 of rtol 1e-3 / atol 1e-8, where the
      reference's own float32 numbers sit at 0.87 from float64 (test_model_gradients_match_reference_goldens has the figures)
Value-only breaks of a scratch copy of the library (valid memory, ordinary failures), one run of this file each, tests
failing:
  the softmax without max subtraction                            15  (all twelve of (b), whose logits reach 100: NaN in T; both
      of (c); (d) at (64, 128), whose inputs are (b)'s.  (a), the engine and the plugin run at logits of a few units and pass)
  the backward ignoring its bitmap (every row is live)           18  ((b) but n = 1, whose row sets all name row 0: gX written
      and NaN read off the bitmap; the two-step and the store_grad tests of (f) at every K; both trajectories of (g).  The
      Adam-state tests of (f) are fed the engine's own gradients and pass)
  the last row slice left out of gW                              13  ((b) at n >= 65 — up to 64 rows are one slice, which the
      break keeps; the two-step tests of (f); in (g) both gradient tests and both trajectories)
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import bigcf_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
D, K = 64, 128
STREAMS = [(2024, 3), (0x9E3779B97F4A7C15, 11)]  # (seed, stream); the second seed does not fit 32 bits


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


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


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


def _bits(t):
    return t.view(torch.int32)


def _ws(ops):
    from idgrec_amd import native

    return torch.empty(int(native.lib.idg_intent_bwd_workspace_bytes(D, K)) // 4, device="cuda")


# ============================================================================================================ (a) the noise
def test_noise_out_is_the_noise_used_and_is_standard_normal(ops):
    n = 32833
    rng = _rng("noise")
    X, W, gF, gT = _randn(rng, (n, D), 0.3), _randn(rng, (D, K), 0.2), _randn(rng, (n, D)), _randn(rng, (n, D))
    seed, sid = STREAMS[1]
    ws = _ws(ops)
    F1, T1, Z = _nan(n, D), _nan(n, D), _nan(n, D)
    ops.intent_fwd_raw(X, W, T1, F1, seed=seed, stream_id=sid, noise_out=Z)
    assert torch.isfinite(Z).all() and torch.isfinite(F1).all()
    F2, T2 = _nan(n, D), _nan(n, D)
    ops.intent_fwd_raw(X, W, T2, F2, noise=Z)
    assert torch.equal(F1, F2) and torch.equal(T1, T2), "the forward fed noise_out gives other bits than the generated noise"
    gX1, gW1, gX2, gW2 = _nan(n, D), _nan(D, K), _nan(n, D), _nan(D, K)
    ops.intent_bwd_raw(gF, gT, None, X, W, gX1, gW1, seed=seed, stream_id=sid, ws=ws)
    ops.intent_bwd_raw(gF, gT, None, X, W, gX2, gW2, noise=Z, ws=ws)
    assert torch.isfinite(gX1).all() and torch.isfinite(gW1).all()
    assert torch.equal(gX1, gX2) and torch.equal(gW1, gW2), "the backward regenerates other noise than the forward used"
    # the stand-alone generator (any width) draws the same numbers; draws are indexed by the GLOBAL row
    assert torch.equal(ops.intent_noise_raw(_nan(n, D), seed, sid), Z)
    Zs, Fs, Ts = _nan(200, D), _nan(200, D), _nan(200, D)
    ops.intent_fwd_raw(X[37:237], W, Ts, Fs, row0=37, seed=seed, stream_id=sid, noise_out=Zs, base_row=37)
    assert torch.equal(Zs, Z[37:237]) and torch.equal(Fs, F1[37:237]) and torch.equal(Ts, T1[37:237])
    assert torch.equal(ops.intent_noise_raw(_nan(5, 32), seed, sid, base_row=7), Z[7:12, :32])
    # other streams, seeds and rows: other draws
    for other in ((seed, sid + 1), (seed + 1, sid)):
        Zo = ops.intent_noise_raw(_nan(n, D), *other)
        assert float((Zo == Z).float().mean()) < 1e-3
    assert not torch.equal(Z[0], Z[1]) and not torch.equal(Z[:, 0], Z[:, 1])
    N = Z.numel()
    mean, var = float(Z.double().mean()), float(Z.double().var())
    print("  N = %d draws: mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)" % (N, mean, 5 / N ** 0.5, var - 1, 5 * (2 / N) ** 0.5))
    assert abs(mean) <= 5 / N ** 0.5 and abs(var - 1) <= 5 * (2 / N) ** 0.5


# ======================================================================================= (b) forward and backward vs float64
LAYER_N = [1, 63, 64, 65, 129, 64 * 512 + 1]  # 32,769 rows: 513 tiles — more than either kernel's persistent workgroups
LDX, LDT_, LDF, LDG = 72, 80, 68, 76            # leading dimensions wider than d (multiples of 4)


def _row_sets(rng, n):
    """None (every row), a random 5 % (at least one row), and rows 0 and n - 1 only — as offsets from row0."""
    some = np.unique(rng.choice(n, max(1, n // 20), replace=False))
    return [("all rows", None), ("5% of rows", some), ("rows 0, n-1", np.unique([0, n - 1]))]


def _case(key, n):
    """Clean inputs of n rows: X (one all-zero row when n > 1), W scaled so that max |X . W| = 100, Z, gF, gT."""
    rng = _rng(key, n)
    X, W = _randn(rng, (n, D), 0.3), _randn(rng, (D, K), 0.2)
    if n > 1:
        X[n // 2] = 0
    W = (W * (100.0 / float((X.double() @ W.double()).abs().max()))).contiguous()
    return rng, X, W, _randn(rng, (n, D)), _randn(rng, (n, D)), _randn(rng, (n, D))


def _panel(clean, row0, flags, ld):
    """A NaN-filled [row0 + n + 3, ld] panel holding `clean` at the flagged rows of row0 .. row0 + n - 1, columns 0 .. d - 1."""
    n = clean.shape[0]
    P = _nan(row0 + n + 3, ld)
    P[row0:row0 + n, :D] = torch.where(flags[:, None], clean, torch.full_like(clean, NAN))
    return P


def _untouched(after, before, row0, flags):
    """Every bit of the panel but columns 0 .. d - 1 of the flagged rows is what it was."""
    a = _bits(after).clone()
    rows = row0 + torch.nonzero(flags).flatten()
    a[rows, :D] = _bits(before)[rows, :D]
    return torch.equal(a, _bits(before))


@pytest.mark.parametrize("row0", [0, 37])
@pytest.mark.parametrize("n", LAYER_N)
def test_intent_kernels_vs_float64(ops, n, row0):
    rng, X, W, Z, gF, gT = _case("layer", n)
    S = X.double() @ W.double()
    assert abs(float(S.abs().max()) - 100.0) < 1e-3  # exp(100) overflows float32: the softmax must subtract the row maximum
    if n > 1:
        assert float(S[n // 2].abs().max()) == 0  # the zero row: uniform P
    F64_, T64_ = ref.intent64(X, W, Z)
    F32_, T32_ = ref.intent64(X, W, Z, dtype=F32)
    ws = _ws(ops)
    N = row0 + n + 3
    for rows_name, rows in _row_sets(rng, n):
        tag = "n=%d row0=%d %s" % (n, row0, rows_name)
        flags = ref._flags(None if rows is None else dev(rows), n, "cuda")
        # the bitmap is indexed by the global row; bits outside row0 .. row0 + n - 1 are set and must not matter
        stray = ([row0 - 1] if row0 else []) + [row0 + n, row0 + n + 2]
        bitmap = None if rows is None else _bitmap(N, np.concatenate([row0 + rows, stray]))
        Xp, Zp = _panel(X, row0, flags, LDX), _panel(Z, row0, flags, D)
        Tp, Fp, Zo = _nan(N, LDT_), _nan(N, LDF), _nan(N, D)
        before = [t.clone() for t in (Tp, Fp, Zo)]
        ops.intent_fwd_raw(Xp[:, :D], W, Tp[:, :D], Fp[:, :D], row0=row0, nrows=n, rows_bitmap=bitmap, noise=Zp, noise_out=Zo)
        for got, was, name in zip((Tp, Fp, Zo), before, ("T", "F", "noise_out")):
            assert _untouched(got, was, row0, flags), "%s: %s was written off the flagged rows" % (tag, name)
            assert torch.isfinite(got[row0:row0 + n, :D][flags]).all(), "%s: %s is not finite at a flagged row" % (tag, name)
        assert torch.equal(Zo[row0:row0 + n][flags], Z[flags])
        _check(tag + " T", Tp[row0:row0 + n, :D][flags], T64_[flags], T32_[flags])
        _check(tag + " F", Fp[row0:row0 + n, :D][flags], F64_[flags], F32_[flags])
        gFp, gTp = _panel(gF, row0, flags, LDG), _panel(gT, row0, flags, LDT_)
        # gT_in with a bitmap of its own: every other flagged row; NaN at the rest, which count as zero
        sub = flags & (torch.arange(n, device="cuda") % 2 == 0)
        gTs, gt_sub = _panel(gT, row0, sub, LDT_), torch.where(sub[:, None], gT, torch.zeros_like(gT))
        sub_bits = _bitmap(N, (row0 + torch.nonzero(sub).flatten()).cpu().numpy())
        for g_name, gt_panel, gt, gt_rows in (("gF+gT", gTp, gT, None), ("gF", None, None, None), ("gF+gT@half", gTs, gt_sub, sub_bits)):
            what = "%s %s" % (tag, g_name)
            gXp, gW = _nan(N, LDF), _nan(D, K)
            was = gXp.clone()
            ws.fill_(NAN)
            ops.intent_bwd_raw(gFp[:, :D], None if gt_panel is None else gt_panel[:, :D], bitmap, Xp[:, :D], W, gXp[:, :D], gW,
                               row0=row0, nrows=n, noise=Zp, ws=ws, gt_rows=gt_rows)
            assert _untouched(gXp, was, row0, flags), what + ": gX was written off the flagged rows"
            assert torch.isfinite(gW).all(), what + ": NaN in gW (memory that must not be read, or a slice never written)"
            gx = gXp[row0:row0 + n, :D][flags]
            assert torch.isfinite(gx).all(), what + ": NaN in gX"
            r64, r32 = ref.intent_grads64(X, W, Z, gF, gt, flags), ref.intent_grads64(X, W, Z, gF, gt, flags, dtype=F32)
            _check(what + " gX", gx, r64[0][flags], r32[0][flags])
            _check(what + " gW", gW, r64[1], r32[1])


# ================================================================================================================ (c) run to run
@pytest.mark.parametrize("n", [129, 64 * 512 + 1])
def test_two_runs_give_equal_bits(ops, n):
    rng, X, W, Z, gF, gT = _case("again", n)
    bitmap = _bitmap(n, _row_sets(rng, n)[1][1])
    seed, sid = STREAMS[0]
    ws = _ws(ops)
    outs = []
    for _ in range(2):
        T, F, gX, gW = _nan(n, D), _nan(n, D), torch.zeros(n, D, device="cuda"), _nan(D, K)
        ws.fill_(NAN)
        ops.intent_fwd_raw(X, W, T, F, seed=seed, stream_id=sid)
        ops.intent_bwd_raw(gF, gT, bitmap, X, W, gX, gW, seed=seed, stream_id=sid, ws=ws)
        outs.append((T, F, gX, gW))
    for a, c, name in zip(outs[0], outs[1], ("T", "F", "gX", "gW")):
        assert torch.isfinite(a).all() and torch.equal(a, c), name


# ===================================================================================================== (d) the differentiable path
def test_autograd_at_64_128_is_the_raw_calls_bit_for_bit(ops):
    n, row0, (seed, sid) = 130, 37, STREAMS[1]
    rng, X, W, Z, gF, gT = _case("autograd", n)
    for noise in (None, Z):
        x, w = X.clone().requires_grad_(True), W.clone().requires_grad_(True)
        F, T = ops.intent_mix(x, w, row0=row0, stream=(seed, sid), noise=noise)
        torch.autograd.backward([F, T], [gF, gT])
        F0, T0, gX, gW = _nan(n, D), _nan(n, D), _nan(n, D), _nan(D, K)
        ops.intent_fwd_raw(X, W, T0, F0, row0=row0, noise=noise, seed=seed, stream_id=sid, base_row=row0)
        ops.intent_bwd_raw(gF, gT, None, X, W, gX, gW, row0=row0, noise=noise, seed=seed, stream_id=sid, base_row=row0)
        assert torch.equal(F.detach(), F0) and torch.equal(T.detach(), T0)
        assert torch.equal(x.grad, gX) and w.grad.shape == (D, K) and torch.equal(w.grad, gW)
    # only F used (the BPR term alone): gT absent
    x, w = X.clone().requires_grad_(True), W.clone().requires_grad_(True)
    F, _ = ops.intent_mix(x, w, row0=row0, stream=(seed, sid))
    F.backward(gF)
    gX, gW = _nan(n, D), _nan(D, K)
    ops.intent_bwd_raw(gF, None, None, X, W, gX, gW, row0=row0, seed=seed, stream_id=sid, base_row=row0)
    assert torch.equal(x.grad, gX) and torch.equal(w.grad, gW)
    # the default stream is the next one of the device seed's sequence: two calls, two draws
    ops.reset_noise_stream()
    a, c = ops.intent_mix(X, W)[0], ops.intent_mix(X, W)[0]
    assert not torch.equal(a, c)


def test_autograd_at_32_16_vs_float64(ops):
    """No kernel at this width: torch operators, with the Z of idg_intent_noise_f32 (the generator's, at the global rows)."""
    n, d, k, row0, (seed, sid) = 257, 32, 16, 37, STREAMS[0]
    rng = _rng("narrow", n)
    X, W, gF, gT = _randn(rng, (n, d), 0.3), _randn(rng, (d, k), 0.5), _randn(rng, (n, d)), _randn(rng, (n, d))
    Z = ops.intent_noise_raw(_nan(n, d), seed, sid, base_row=row0)
    assert torch.equal(Z, ops.intent_noise_raw(_nan(row0 + n, d), seed, sid)[row0:])
    x, w = X.clone().requires_grad_(True), W.clone().requires_grad_(True)
    F, T = ops.intent_mix(x, w, row0=row0, stream=(seed, sid))
    torch.autograd.backward([F, T], [gF, gT])
    F64_, T64_ = ref.intent64(X, W, Z)
    F32_, T32_ = ref.intent64(X, W, Z, dtype=F32)
    _check("(32, 16) T", T.detach(), T64_, T32_)
    _check("(32, 16) F", F.detach(), F64_, F32_)
    r64, r32 = ref.intent_grads64(X, W, Z, gF, gT), ref.intent_grads64(X, W, Z, gF, gT, dtype=F32)
    _check("(32, 16) gX", x.grad, r64[0], r32[0])
    _check("(32, 16) gW", w.grad, r64[1], r32[1])


# ===================================================================================================== (e) the self-contrast InfoNCE
@pytest.mark.parametrize("B", [96, 30])  # (B % 4 == 0: the matrix-core stages; 30: the SIMT ones)
def test_infonce_pair_with_one_panel_as_both_views(ops, B):
    """get_InfoNCE_loss(a, a, t) over the raw user rows and over the raw positive rows: view1 is view2, and ONE panel as g1
    and g2 receives the sum of both arguments' gradients (idg_ssl.hip: the views are only read — the normalise kernel's
    __restrict__ pointers are never written through — and g1 == g2 takes ssl_final_kernel's both_views branch, view 1's
    rows first).  Duplicate ids: every occurrence is a row of the in-batch matrix, their gradients add up in the panel row."""
    U, I, d, t = 300, 250, 64, 0.2
    rng = _rng("self", B)
    view = _randn(rng, (U + I, d), 0.5)
    users, pos = dev(rng.integers(0, U, B).astype(np.int64)), dev(rng.integers(0, I, B).astype(np.int64))
    users[1], users[5], pos[1], pos[7] = users[0], users[3], pos[0], pos[2]
    g = torch.zeros_like(view)
    loss = ops.infonce_pair_raw(view, view, users, pos, U, t, g1=g, g2=g, dedup=False).clone()
    res = {}
    for name, dtype in (("64", F64), ("32", F32)):
        x = view.to(dtype).clone().requires_grad_(True)
        with ref.deterministic():
            terms = torch.stack([ref.infonce64(x[users], x[users], t, dtype), ref.infonce64(x[U + pos], x[U + pos], t, dtype)])
            (gx,) = torch.autograd.grad(terms.sum(), x)
        res[name] = (terms.detach(), gx)
    tag = "self InfoNCE B=%d" % B
    for k, name in enumerate(("users", "positives")):
        _check("%s loss %s" % (tag, name), loss[k], res["64"][0][k], res["32"][0][k])
    _check(tag + " summed gradient", g, res["64"][1], res["32"][1])
    assert torch.equal(g.abs().sum(dim=1) == 0, res["64"][1].abs().sum(dim=1) == 0), tag + ": other rows receive gradient"
    # STORED (accumulate = False) into a NaN panel: the named rows hold the same bits, every other row is the NaN it was;
    # ADDED (accumulate = True) on top of a panel: that panel plus the gradient, scaled
    gs = _nan(U + I, d)
    ops.infonce_pair_raw(view, view, users, pos, U, t, g1=gs, g2=gs, dedup=False, accumulate=False)
    named = g.abs().sum(dim=1) != 0
    assert torch.equal(gs[named], g[named]) and torch.isnan(gs[~named]).all()
    base = _randn(rng, (U + I, d))
    ga = base.clone()
    ops.infonce_pair_raw(view, view, users, pos, U, t, g1=ga, g2=ga, dedup=False, grad_scale=0.2, accumulate=True)
    assert torch.equal(ga[~named], base[~named])
    scale = float(np.float32(0.2))
    _check(tag + " added, scaled by 0.2", ga, base.double() + scale * res["64"][1], base + scale * res["32"][1])
    # the differentiable form with the same tensor twice: autograd adds the two arguments' gradients
    v = view.clone().requires_grad_(True)
    ops.infonce_pair(v, v, users, pos, U, t, dedup=False).backward()
    _check(tag + " under autograd", v.grad, res["64"][1], res["32"][1])


# ================================================================================================================ (f) the engine
REG, LR, SSL, TEMP = float(np.float32(1e-4)), 1e-3, 0.2, 0.2
ENGINE_K = [2, 1, 3]
_engine_runs = {}
_graphs = {}


@pytest.fixture(scope="module")
def golden_bigcf():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "bigcf_small.npz"), allow_pickle=False))
    g.update(np.load(os.path.join(ROOT, "tests", "golden", "bigcf_small_one.npz"), allow_pickle=False))
    return g


def _graph(ops, golden_small):
    if "g" not in _graphs:
        g = golden_small
        n = int(g["num_users"]) + int(g["num_items"])
        _graphs["g"] = (ops.Graph(g["adj_indptr"], g["adj_indices"], g["adj_data"], n, n),
                        ref.dense_operator(g["adj_indptr"], g["adj_indices"], g["adj_data"], (n, n), device="cuda"))
    return _graphs["g"]


def _engine_run(ops, golden_small, golden_bigcf, K):
    """Two training steps with store_grad and known noise streams — the B = 96 batch with duplicate users and items, then a
    256-row one — every step next to step64 in float64 and float32 FROM THE ENGINE'S OWN PARAMETERS read back before the step
    and the Z of idg_intent_noise_f32 for the step's stream; then the same two steps without store_grad.  U = 300: the
    user / item boundary falls inside the fifth 64-row tile."""
    if K in _engine_runs:
        return _engine_runs[K]
    from idgrec_amd.bigcf import BigcfEngine

    G, A64 = _graph(ops, golden_small)
    U, I = int(golden_small["num_users"]), int(golden_small["num_items"])
    n = U + I
    rng = _rng("engine", K)
    xav = lambda r, c: dev(rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32))  # noqa: E731
    P0 = torch.cat([xav(U, D), xav(I, D)])
    W0 = (xav(D, 128), xav(D, 128))
    batches = [tuple(dev(golden_bigcf["batch"][:, c]) for c in range(3)),
               tuple(dev(golden_bigcf["traj_batches"][256:512, c]) for c in range(3))]  # ([:256] contains the B = 96 batch)
    streams = [STREAMS[1], (77, 5)]

    def make(store_grad):
        return BigcfEngine(G, U, I, P0.clone(), W0, K, reg_lambda=REG, ssl_lambda=SSL, temperature=TEMP, lr=LR, store_grad=store_grad)

    eng = make(True)
    SW0 = eng.SW.clone()
    steps = []
    for s, (users, pos, neg) in enumerate(batches):
        P_before, (Wu, Wi) = eng.P.clone(), (v.clone() for v in eng.intent_views())
        loss = eng.train_step(users, pos, neg, stream=streams[s]).clone()
        st = dict(loss=loss, GRAD=eng.GRAD.clone(), SG=eng.SG.clone(), P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(),
                  SW=eng.SW.clone(), SM=eng.SM.clone(), SV=eng.SV.clone(), F=eng.F.clone(), T=eng.T.clone())
        Z = ops.intent_noise_raw(_nan(n, D), *streams[s])
        for name, dtype in (("64", F64), ("32", F32)):
            losses, _, (gE0, gWu, gWi), F_, T_ = ref.step64(A64, P_before, Wu, Wi, users, pos, neg, Z, K, REG, SSL, TEMP, U, dtype=dtype)
            st["loss" + name], st["GRAD" + name], st["F" + name], st["T" + name] = losses, gE0, F_, T_
            st["SG" + name] = torch.cat([gWu.reshape(-1), gWi.reshape(-1)])
        steps.append(st)
    assert eng.step_count == 2
    lean = make(False)
    for s, (users, pos, neg) in enumerate(batches):
        lean.train_step(users, pos, neg, stream=streams[s])
    run = dict(P0=P0, SW0=SW0, steps=steps, lean=tuple(t.clone() for t in (lean.P, lean.M, lean.V, lean.SW, lean.SM, lean.SV)))
    torch.cuda.synchronize()
    _engine_runs[K] = run
    return run


@pytest.mark.parametrize("K", ENGINE_K)
def test_engine_two_steps_vs_float64(ops, golden_small, golden_bigcf, K):
    """The second step's batch names other rows than the first's: rows of step 1 leaking into step 2 — through gF, through
    gT (stored at the user and positive rows only), through gX, through the regulariser's panel that the last product takes
    as its masked addend — would show in its gradients."""
    run = _engine_run(ops, golden_small, golden_bigcf, K)
    per = D * 128
    for s, st in enumerate(run["steps"], 1):
        tag = "engine K=%d step %d" % (K, s)
        assert torch.isfinite(st["loss"]).all() and torch.isfinite(st["GRAD"]).all() and torch.isfinite(st["SG"]).all()
        for k, name in enumerate(("bpr", "reg", "ssl")):
            _check("%s loss %s" % (tag, name), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " F", st["F"], st["F64"], st["F32"])
        _check(tag + " T", st["T"], st["T64"], st["T32"])
        _check(tag + " GRAD", st["GRAD"], st["GRAD64"], st["GRAD32"])
        assert torch.equal(st["GRAD"].abs().sum(dim=1) == 0, st["GRAD64"].abs().sum(dim=1) == 0), tag + ": other rows receive gradient"
        for i, name in enumerate(("gW_u", "gW_i")):
            _check("%s %s" % (tag, name), st["SG"][i * per:(i + 1) * per], st["SG64"][i * per:(i + 1) * per], st["SG32"][i * per:(i + 1) * per])
    rows = [set(np.concatenate([b[:, 0], 300 + b[:, 1], 300 + b[:, 2]]).tolist())
            for b in (golden_bigcf["batch"], golden_bigcf["traj_batches"][256:512])]
    assert len(rows[0] - rows[1]) > 20
    if K == 1:
        a, c = (st["GRAD64"].abs().sum(dim=1) > 0 for st in run["steps"])
        assert bool((a & ~c).any()) and bool((c & ~a).any())


@pytest.mark.parametrize("K", ENGINE_K)
def test_engine_adam_state_after_each_step(ops, golden_small, golden_bigcf, K):
    """tests/test_gpu_gccf.py::test_engine_adam_state_after_each_step: on the embedding panel (Adam in the last product's
    epilogue) and on the flat buffer [W_u | W_i] (one launch): exp_avg, exp_avg_sq within 4 * 2^-24 of their largest entry,
    the parameters within 4 ulp of their largest entry, against the float64 recurrence fed the engine's own two gradients
    from the float32 initial values."""
    run = _engine_run(ops, golden_small, golden_bigcf, K)
    for what, W0, gk, wk, mk, vk in (("panel", run["P0"], "GRAD", "P", "M", "V"), ("intents", run["SW0"], "SG", "SW", "SM", "SV")):
        want = ref.adam64(W0, [st[gk] for st in run["steps"]], lr=LR)
        for s, (st, (W, M, V)) in enumerate(zip(run["steps"], want), 1):
            for name, got, w in (("exp_avg", st[mk], M), ("exp_avg_sq", st[vk], V)):
                e = float((got.double() - w).abs().max() / w.abs().max())
                print("  K=%d %s step %d %s: %.2f * 2^-24 of max" % (K, what, s, name, e * 2.0 ** 24))
                assert e <= 4 * 2.0 ** -24, (what, name, s, e)
            wmax = float(W.abs().max())
            ulp = float(np.spacing(np.float32(wmax)))
            e = float((st[wk].double() - W).abs().max())
            print("  K=%d %s step %d parameters: %.2f ulp of max |W| = %.3f" % (K, what, s, e / ulp, wmax))
            assert e <= 4 * ulp, (what, s, e / ulp)
        assert not torch.equal(run["steps"][0][wk], run["steps"][1][wk])


@pytest.mark.parametrize("K", ENGINE_K)
def test_engine_without_stored_gradient_is_bit_identical(ops, golden_small, golden_bigcf, K):
    run = _engine_run(ops, golden_small, golden_bigcf, K)
    last = run["steps"][-1]
    for got, name in zip(run["lean"], ("P", "M", "V", "SW", "SM", "SV")):
        assert torch.equal(got, last[name]), name


# ================================================================================================================ (g) the plugin
PARAMS = ("user_embedding", "item_embedding", "user_intent", "item_intent")


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "BIGCF.txt"), "BIGCF")
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


def _model(tmp_path, golden_small, K):
    import utility.utility_function.tools as tools
    from models.BIGCF import BIGCF

    cfg = _cfg(GCN_layer=K)
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = BIGCF(cfg, data, torch.device("cuda")).to("cuda")
    return cfg, m, {p: getattr(m, p).weight for p in PARAMS}


SETTINGS = [("def", 2), ("one", 1)]


@pytest.mark.parametrize("tag,K", SETTINGS)
def test_model_losses_and_rating_match_reference_goldens(ops, tag, K, tmp_path, golden_small, golden_bigcf):
    """Losses and rating at the tolerances of tests/test_gpu_gccf.py::test_model_matches_reference_goldens (which cites
    tests/test_gpu_models.py::test_ngcf_vs_reference); the reference's recorded noise is injected."""
    g = golden_bigcf
    za, zb = dev(g["noise_a"]), dev(g["noise_b"])
    cfg, m, prm = _model(tmp_path, golden_small, K)
    assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
    for p in PARAMS:  # same torch RNG order as the reference's constructor
        assert np.array_equal(prm[p].detach().cpu().numpy(), g["init_" + p]), p
    b = torch.from_numpy(g["batch"]).cuda()
    out = m.aggregate(noise=za)
    assert [tuple(t.shape) for t in out] == [(300, 64), (250, 64), (300, 64), (250, 64)]
    m.noise_source = lambda: za
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 3
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-4)
    m.eval()
    users = torch.from_numpy(g["rating_users"]).cuda()
    np.testing.assert_allclose(m.get_rating_for_test(users, noise=zb).cpu().numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    # evaluation draws its own noise otherwise: one draw per pass (cached while the weights are frozen), another the next pass
    m.noise_source = None
    r1, r2 = m.get_rating_for_test(users), m.get_rating_for_test(users)
    assert torch.equal(r1, r2) and torch.isfinite(r1).all() and not torch.equal(r1.cpu(), torch.from_numpy(g[tag + "_rating"]))
    m.train()
    m.eval()
    assert not torch.equal(m.get_rating_for_test(users), r1)
    assert m.topk_for_test(users, 10).shape == (32, 10)


@pytest.mark.parametrize("tag,K", SETTINGS)
def test_model_gradients_match_reference_goldens(ops, tag, K, tmp_path, golden_small, golden_bigcf):
    """Every .grad of forward() + backward() at the tolerances of tests/test_gpu_models.py::test_ngcf_vs_reference: rtol 1e-3
    with atol 1e-8 on the two tables and 1e-7 on the intent matrices.

    The tolerance is that of the other plugins' fixtures, whose table gradients are an order of magnitude smaller; here the
    reference's OWN float32 gradient sits up to 0.87 of the tolerance from the float64 statement (tests/bigcf_ref64.py, which
    tests/test_bigcf_host.py holds to it), so the path under test has a tenth of the tolerance to itself at that element.
    Measured on an MI355X, worst element of each of the four gradients as a share of the tolerance: `def` 0.48 / 0.89 / 0.20 /
    0.01, `one` 0.09 / 0.81 / 0.18 / 0.01 (the reference from float64: 0.48 / 0.87 / 0.20 / 0.01 and 0.10 / 0.82 / 0.18 / 0.01).
    With the five InfoNCE terms of forward() evaluated in float32 on this library's kernels `def` missed it
    by one element of 53,584: item_embedding.grad[65, 7], float64 1.4911e-6, the reference 1.4810e-6, that path 1.4936e-6
    (1.10); stage by stage, 2.3e-9 of its 2.5e-9 came from those terms' gradients, which is why forward() evaluates them in
    float64 (models/BIGCF.py).  The figures of a run — this path's, the reference's and the float64 statement's value of every
    element outside — are printed before the assertion."""
    g = golden_bigcf
    za = dev(g["noise_a"])
    cfg, m, prm = _model(tmp_path, golden_small, K)
    b = torch.from_numpy(g["batch"]).cuda()
    m.zero_grad()
    ll = m(b[:, 0], b[:, 1], b[:, 2], noise=za)
    sum(ll).backward()
    _, A64 = _graph(ops, golden_small)
    E0 = torch.cat([dev(g["init_user_embedding"]), dev(g["init_item_embedding"])])
    r64 = ref.step64(A64, E0, dev(g["init_user_intent"]), dev(g["init_item_intent"]), b[:, 0], b[:, 1], b[:, 2], za, K,
                     float(cfg["reg_lambda"]), float(cfg["ssl_lambda"]), float(cfg["ssl_temperature"]), 300)[2]
    g64 = dict(zip(PARAMS, (r64[0][:300], r64[0][300:], r64[1], r64[2])))
    for p, atol in zip(PARAMS, (1e-8, 1e-8, 1e-7, 1e-7)):
        mine, want = prm[p].grad.cpu().numpy(), g["%s_grad_%s" % (tag, p)]
        tol = atol + 1e-3 * np.abs(want)
        ratio, ratio_ref = np.abs(mine - want) / tol, np.abs(g64[p].cpu().numpy() - want) / tol
        print("grad %s: %d of %d elements outside rtol 1e-3 / atol %g, worst %.2f of the tolerance (the reference from float64: "
              "%.2f), max |g| %.3g" % (p, int((ratio > 1).sum()), ratio.size, atol, ratio.max(), ratio_ref.max(), np.abs(want).max()))
        for r, c in zip(*np.nonzero(ratio > 1)):
            print("   [%d, %d]: this path %.6e, the reference %.6e, float64 %.6e" % (r, c, mine[r, c], want[r, c], float(g64[p][r, c])))
    for p, atol in zip(PARAMS, (1e-8, 1e-8, 1e-7, 1e-7)):
        np.testing.assert_allclose(prm[p].grad.cpu().numpy(), g["%s_grad_%s" % (tag, p)], rtol=1e-3, atol=atol, err_msg=p)


@pytest.mark.parametrize("tag,K", SETTINGS)
def test_model_fused_steps_match_reference_trajectory(ops, tag, K, tmp_path, golden_small, golden_bigcf):
    """Three fused steps against the reference's own Adam trajectory, at the tolerances of
    tests/test_gpu_lgcnpp.py::test_model_matches_reference_goldens; the recorded noise of every step is injected."""
    g = golden_bigcf
    za, zb = dev(g["noise_a"]), dev(g["noise_b"])
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    cfg, m, prm = _model(tmp_path, golden_small, K)
    assert m.fused_step_available()
    seq = iter((za, zb, za))
    m.noise_source = lambda: next(seq)
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 3), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    # (the trajectory criterion of tests/test_gpu_lgcnpp.py: Adam divides by sqrt(v), so where a gradient is of the order of
    # its own rounding error a last-place difference moves the element visibly)
    for p in PARAMS:
        mine, want = prm[p].detach().cpu().numpy(), g["%s_traj_%s" % (tag, p)]
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("trajectory %s: off %.3g, max %.3g" % (p, off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, (p, off.mean())
        assert np.abs(mine - want).max() < 1e-4, (p, np.abs(mine - want).max())
    assert all(int(opt.state[q]["step"]) == 3 for q in m.parameters())


def test_model_at_other_widths_trains_through_autograd(ops, tmp_path, golden_small):
    """intent_size = 16: no kernel at that width and no fused step; the differentiable path gives finite losses and a gradient
    for every parameter."""
    import utility.utility_function.tools as tools
    from models.BIGCF import BIGCF

    rng = _rng("batch")
    b = [dev(rng.integers(0, hi, 128).astype(np.int64)) for hi in (300, 250, 250)]
    cfg = _cfg(intent_size=16)
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = BIGCF(cfg, data, torch.device("cuda")).to("cuda")
    assert not m.fused_step_available()
    m.train()
    ll = m(*b)
    sum(ll).backward()
    assert len(ll) == 3 and all(torch.isfinite(x).all() for x in ll)
    for name, prm in m.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0, name
