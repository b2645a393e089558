"""NGCF's layer kernels (idg_dense.hip: transform, tail, their backward forms, idg_ngcf_wgrad_f32; idg_ngcf.hip: the fused
d = 64 layer kernels) and the fused step (idgrec_amd/ngcf.py) against float64, across their dispatch.  The reference
statement is tests/ngcf_ref64.py, pinned to the reference's own numbers and to splitmix64 by tests/test_ngcf_ref.py.

  (a) the message-dropout mask of every tail form and of the fused forward kernel, bit for bit against ngcf_ref64.keep_mask;
  (b) idg_ngcf_tail_ex_f32 / idg_ngcf_tail_bwd_ex_f32: vector forms (d = 32, 64, 128, 256) and the one-wave-per-row form,
      S2 given or NULL, gE / gN / both, no bitmap / a 5 % bitmap / first and last row only, N written into and gN read from
      a slot of a wider panel, fully dropped rows, clamped rows, exact zeros of the pre-activation, NaN in unread memory;
  (c) idg_ngcf_transform_f32 / _bwd_f32 at every accepted width class, n below one row tile, grids below their minimum
      and the persistent walk past one tile per wave;
  (d) idg_ngcf_wgrad_f32 with fewer rows than slices;
  (e) idg_ngcf_layer_fwd_f32 / _bwd_f32 against float64 AND bit for bit against the chain, 1, 2 and more than 512 blocks;
  (f) NgcfEngine, fused (d = 64) and chain (d = 128, 256, IDG_NGCF_LAYER=0), two steps: losses, every gradient, Adam state.

One tolerance rule throughout (egcf_ref64.errors / band): with scale = max |ref64| of the tensor compared,
    e_kernel = max |kernel - ref64| / scale   <=   max(4 e_f32, 8 * 2^-24),   e_f32 = max |float32 composition - ref64| / scale
where the float32 composition is ngcf_ref64's same expressions in float32, run in the same test; both numbers are printed
(pytest -s).  Clamped rows (||E|| = 0: the Jacobian of normalize is I / 1e-12) are compared on their own scale.
Bit claims (torch.equal) where the code makes them: the mask, untouched memory, run to run, fused layer versus chain for
E, N, g_side, g_ego, slot versus contiguous panel, store_grad on versus off.

Kernel and reference share one operator: the graph's float32 values (dense_operator), the mask and its float32 scale
(keep_mask), the float32 roundings of the slope and of reg_lambda (what the C ABI's `float` arguments carry).

Measured on an MI355X (185 tests, 8.3 .. 10.0 s for the whole file once the library is loaded), e_kernel / e_f32 over all
comparisons of a group, worst e_kernel / band:
  (a) exact: every E equals keep_mask bit for bit (11 tests, 77 panels)
  (b) 2.9e-9 .. 1.1e-6 / 2.9e-9 .. 2.2e-6 (0.39: d = 100, n = 257, gN at rows 0 and n - 1), 2290 comparisons, clamped rows
      included (on their own scale); the 312 of them on rows of 4 and 7 features with gN: six above the plain band, at
      1.04 .. 1.60 times (d = 4, n = 1 and 3; d = 7, n = 63 with three flagged rows), every element at most 0.33 of
      max(band, argued bound) — see _check_short_rows
  (c) 1.3e-7 .. 5.6e-7 / 5.7e-8 .. 5.4e-7 (0.72: forward n = 1, (64, 32))
  (d) 0 .. 2.1e-7 / 0 .. 9.4e-7 (0.39: n = 511, (64, 64), g b1)
  (e) 4.5e-9 .. 6.7e-7 / 4.5e-9 .. 3.8e-6 (0.66: n = 64, p = 0, gE alone, g_ego), 1072 comparisons
  (f) 1.2e-9 .. 6.8e-6 / 1.2e-9 .. 4.8e-6 (0.54: d = 64, K = 3, step 2, layer 2's g b_gcn); Adam moments at most 2.38 * 2^-24 of
      their largest entry, parameters at most 1.01 ulp of theirs
Met while writing the file, no fault of a kernel: LeakyReLU's kink (see _near_the_kink) — at n = 32,833, p = 0.1 one element of
2.1 million had float32 and float64 pre-activations of opposite sign and g_side sat 4.1e-2 from the reference.
Value-only breaks of a scratch copy of the library, one run of this file each, tests failing:
  keep_scale reading bits 16 ((f + 1) & 3)                                   33  (the generic forms of (a) and (b))
  the e == 0 derivative 0 when kept: vector tail' / generic tail' / fused'    6 / 4 / 2  (exact zeros of (b); clamped row of (e))
  the clamp branch keeping the projection: vector / generic / fused           3 / 1 / 1  (the rows below the clamp that are not zero:
      on an all-zero row this break changes nothing, which is why those rows were added)
  gn_rows ignored in the fused backward                                      27  ((e) but n = 1, whose row sets all name row 0: NaN off the bitmap; (f))
  the bias column sum without its __shfl_xor                                 23  ((e) but n = 1, where odd rows do not exist; (f))
  transform forward dropping the chunks after the first                      23  (d1 = 128, 192 of (c); the chain engines of (f))
  idg_ngcf_wgrad_f32 summing all slices but the last                         16  ((d) but n = 513, whose last slices hold no row; (f))"""
import ctypes as C
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import ngcf_ref64 as ref  # noqa: E402

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
SLOPE = float(np.float32(0.2))
STREAMS = [(1234, 7), ((1 << 32) + 987654321, 3)]  # (seed, stream); the second seed does not fit 32 bits


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


@pytest.fixture(scope="module")
def lib(ops):
    from idgrec_amd import native

    return native.lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _rng(*key):
    return np.random.default_rng(_seed(*key))


def _randn(rng, shape, scale=1.0):
    return dev((rng.standard_normal(shape) * scale).astype(np.float32))


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _p(t, offset=0):
    """Device pointer of a tensor (None: NULL), `offset` floats in."""
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)


def _check(what, got, ref64, f32, scale=None):
    e_k, e_f = ref.errors(got, ref64, f32, scale)
    print("  %-74s e_kernel %.2e  e_f32 %.2e  (%.2f of the band)" % (what, e_k, e_f, e_k / ref.band(e_f)))
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


def _bitmap(n, rows):
    """int32 [ceil(n / 32)] device bitmap with the bits of `rows` set (n % 32 != 0: a partial last word)."""
    rows = np.asarray(rows, dtype=np.int64)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return dev(words.view(np.int32))


def ONE():
    return torch.ones((), device="cuda")


def _mask(p, stream, n, d, dtype=F64):
    return ref.keep_mask(p, stream[0], stream[1], n, d, dtype=dtype).cuda()


KINK = 1e-5


def _near_the_kink(t64, terms64):
    """bool [n]: rows with an element 0 < |t| < 1e-5 * (the sum of the absolute values of t's terms).  LeakyReLU' jumps from
    `slope` to 1 at t = 0 and the kernels read the side from the sign of their own float32 E; a float32 evaluation of t
    (up to 2 * 64 + 3 roundings: at most 8e-6 of that sum, typically 1e-7) may land on the other side there, and the
    element's gradient is then 0.8 g off in ANY correct float32 evaluation (met at n = 32,833: one of 2.1 million
    elements, g_side 4e-2 off).  Such rows — found from the float64 statement alone, about 100 of 32,833 at d = 64 — are
    given no upstream gradient, so that their gT is 0 on both sides of the kink.  t == 0 exactly (the constructed cases)
    is no such row: there both agree on `slope`."""
    return ((t64.abs() < KINK * terms64) & (t64 != 0)).any(dim=1)


def _short_row_bound(E64, N64, mask, gn, flags, gT64):
    """Per element, the forward error bound of the float32 evaluation of
        gT_f = c_f ((gn_f - dot e_f / ss) / den),   c_f = keep * LeakyReLU',  dot = sum gn_i e_i,  ss = sum e_i^2 over the m kept i:
    dot and ss carry m + 1 roundings each of sum |gn_i e_i| <= ||gn|| ||e|| and of ss, the quotient chain 4 more, so
        |error of dot e_f / ss| <= (2 m + 6) u ||gn|| |y_f|,     y = e / ||e||,  u = 2^-24,
    and the subtraction, the division by den and the two products by c_f add 4 u of each term:
        |error of gT_f| <= u c_f / ||e|| ((2 m + 10) ||gn|| |y_f| + 4 |gn_f|)."""
    u = 2.0 ** -24
    c = mask.to(F64) * torch.where(E64 > 0, 1.0, SLOPE)
    den = E64.norm(dim=1, keepdim=True).clamp_min(1e-300)
    m = (mask != 0).sum(dim=1, keepdim=True).to(F64)
    g = torch.where(flags[:, None], gn.to(F64), torch.zeros((), dtype=F64, device=gn.device))
    return u * c / den * ((2 * m + 10) * g.norm(dim=1, keepdim=True) * N64.abs() + 4 * g.abs()) + 4 * u * gT64.abs()


# ------------------------------------------------------------------------------------------------------ the C ABI calls
def _ok(code, where):
    from idgrec_amd import native

    native.check(code, where)


def tail_fwd(ops, lib, S1, S2, b1, b2, n, d, p, stream, E, N, ldn, slot=0, s1_offset=0):
    _ok(lib.idg_ngcf_tail_ex_f32(_p(S1, s1_offset), _p(S2), _p(b1), _p(b2), n, d, SLOPE, p, stream[0], stream[1], _p(E),
                                 _p(N, slot * d), ldn, ops._stream()), "idg_ngcf_tail_ex_f32")


def tail_bwd(ops, lib, E, gE, gN, ldgn, bitmap, n, d, p, stream, gT, slot=0):
    _ok(lib.idg_ngcf_tail_bwd_ex_f32(_p(E), _p(gE), _p(gN, slot * d), ldgn, _p(bitmap), n, d, SLOPE, p, stream[0], stream[1],
                                     _p(gT), ops._stream()), "idg_ngcf_tail_bwd_ex_f32")


# ============================================================================================================ (a) the mask
MASK_P = [0.1, 0.5, 0.999]
MASK_ELEMS = ((1 << 16) + 3) * 64  # the largest panel of this file


def _mask_runs(d):
    """(n, p, stream): n = 2^16 + 3 (the row term of the mix past 16 bits) once where the panel stays within MASK_ELEMS —
    the widest forms get the most rows that fit — and n = 1027 for every other (p, stream)."""
    big = min((1 << 16) + 3, MASK_ELEMS // d)
    return [(big, 0.5, STREAMS[1])] + [(1027, p, s) for p in MASK_P for s in STREAMS if (p, s) != (0.5, STREAMS[1])]


def _expect_mask(what, E, p, stream, n, d):
    want = _mask(p, stream, n, d, dtype=F32)
    assert E.shape == want.shape
    bad = int((E != want).sum())
    assert torch.equal(E, want), "%s: %d of %d elements differ from keep_mask" % (what, bad, n * d)
    dropped = float((want == 0).float().mean())
    assert abs(dropped - p) < 0.02, (what, dropped)


@pytest.mark.parametrize("d", [32, 64, 128, 256, 48, 100, 4, 7])
def test_mask_of_the_tail_forms_is_the_published_one(ops, lib, d):
    """S1 = 1, S2 = NULL, b = 0: t = 1, so E IS the keep scale or 0.  d = 32 .. 256: keep_scale4 in
    ngcf_tail_fwd_vec_kernel<8, 16, 32, 64>; d = 48, 100, 4, 7: keep_scale in ngcf_tail_fwd_kernel (100: two passes of
    the wave over the row; 7: features that share a mix end mid-group)."""
    b = torch.zeros(d, device="cuda")
    for n, p, stream in _mask_runs(d):
        S1, E, N = torch.ones(n, d, device="cuda"), _nan(n, d), _nan(n, d)
        tail_fwd(ops, lib, S1, None, b, b, n, d, p, stream, E, N, d)
        _expect_mask("tail d=%d n=%d p=%g seed=%d" % (d, n, p, stream[0]), E, p, stream, n, d)


@pytest.mark.parametrize("how", ["ldn=65", "S1 one float in"])
def test_mask_of_the_generic_tail_forced_at_width_64(ops, lib, how):
    """d = 64 falls to the one-wave-per-row form when ldn % 4 != 0 or a panel is not 16-byte aligned: the same mask."""
    d = 64
    b = torch.zeros(d, device="cuda")
    for n, p, stream in _mask_runs(d):
        ldn = 65 if how == "ldn=65" else d
        off = 0 if how == "ldn=65" else 1
        S1 = torch.ones(n * d + 1, device="cuda")
        E, N = _nan(n, d), _nan(n, ldn)
        tail_fwd(ops, lib, S1, None, b, b, n, d, p, stream, E, N, ldn, s1_offset=off)
        _expect_mask("generic tail d=64 %s n=%d p=%g" % (how, n, p), E, p, stream, n, d)
        if ldn > d:
            assert torch.isnan(N[:, d:]).all() and torch.isfinite(N[:, :d]).all()


def test_mask_of_the_fused_forward_kernel_is_the_published_one(ops, lib):
    """idg_ngcf_layer_fwd_f32 with W1 = I, W2 = 0, b = 0, side = 1: the accumulator is exactly 1."""
    d = 64
    W1, W2, b = torch.eye(d, device="cuda"), torch.zeros(d, d, device="cuda"), torch.zeros(d, device="cuda")
    for n, p, stream in _mask_runs(d):
        side, ego = torch.ones(n, d, device="cuda"), _randn(_rng("mask-ego", n), (n, d))
        E, N = _nan(n, d), _nan(n, d)
        _ok(lib.idg_ngcf_layer_fwd_f32(_p(side), _p(ego), _p(W1), _p(W2), _p(b), _p(b), n, d, SLOPE, p, stream[0], stream[1],
                                       _p(E), _p(N), d, ops._stream()), "idg_ngcf_layer_fwd_f32")
        _expect_mask("fused forward n=%d p=%g seed=%d" % (n, p, stream[0]), E, p, stream, n, d)


# ================================================================================================================ (b) the tail
TAIL_D = [4, 7, 32, 48, 64, 100, 128, 256]
TAIL_N = [1, 3, 63, 64, 65, 257]


def _row_sets(rng, n):
    """gn_rows: None (every row), a random 5 % (at least one row), and rows 0 and n - 1 only."""
    some = np.unique(rng.choice(n, max(1, n // 20), replace=False))
    return [("all rows", None), ("5% of rows", some), ("rows 0, n-1", np.unique([0, n - 1]))]


def _check_short_rows(what, got, r64, r32, bound):
    """d = 4, 7 with gN: a row's gradient is what a projection in at most 7 dimensions leaves of gN — a difference of terms
    that may nearly cancel, with no averaging over a long row or (n = 1, 3) over many rows; the kernel's residue and the
    float32 composition's are then two draws of a few roundings, and their ratio is not held by 4.  Measured under the
    plain rule: six misses in the 312 comparisons made here, at 1.04 to 1.60 times the band (d = 4, n = 1: e_kernel
    9.7e-7 against e_f32 1.5e-7 on a scale that is itself the residue; d = 4, n = 3; d = 7, n = 63 with three flagged
    rows), none in the other 1978 of (b).  Every element must instead sit within the band OR within the forward error
    bound of _short_row_bound (at most 24 u ||gN|| / ||E|| per element at d = 7); measured: at most 0.33 of that.  Every other
    comparison of this file keeps the plain rule."""
    e_k, e_f = ref.errors(got, r64, r32)
    scale = float(r64.abs().max())
    err = (got.double() - r64).abs()
    allowed = torch.maximum(bound, torch.full_like(bound, ref.band(e_f) * scale))
    worst = float((err / allowed).max())
    print("  %-74s e_kernel %.2e  e_f32 %.2e  (%.2f of the band; short rows: %.2f of max(band, argued bound))"
          % (what, e_k, e_f, e_k / ref.band(e_f), worst))
    assert worst <= 1.0, "%s: e_kernel %.3e, an element at %.2f times max(band, argued bound)" % (what, e_k, worst)


def _tail_case(ops, lib, d, n, p, with_s2, stream, key="tail", consts=None, extra=None):
    """Forward into slot 2 of a [n, 4d] panel of sentinels (and once more into a contiguous panel: same bits), then the
    backward for gE only / gN only / both times the three row sets, gN read from slot 2 of a [n, 4d] panel whose other
    slots, and whose rows off the bitmap, hold NaN.  consts = (b1, b2, S1) overrides the random inputs."""
    rng = _rng(key, d, n, p, with_s2)
    tag = "%s d=%d n=%d p=%g %s" % (key, d, n, p, "S2" if with_s2 else "S2=NULL")
    if consts is None:
        S1, b1, b2 = _randn(rng, (n, d)), _randn(rng, (d,), 0.3), _randn(rng, (d,), 0.3)
    else:
        b1, b2, S1 = consts
    S2 = _randn(rng, (n, d)) if with_s2 else None
    mask = _mask(p, stream, n, d)
    E, panel = _nan(n, d), torch.full((n, 4 * d), 7.0, device="cuda")
    tail_fwd(ops, lib, S1, S2, b1, b2, n, d, p, stream, E, panel, 4 * d, slot=2)
    assert (panel[:, :2 * d] == 7.0).all() and (panel[:, 3 * d:] == 7.0).all(), tag + ": the panel was written outside the slot"
    N = panel[:, 2 * d:3 * d]
    E64, N64 = ref.tail64(S1, S2, b1, b2, SLOPE, mask)
    E32, N32 = ref.tail64(S1, S2, b1, b2, SLOPE, mask, dtype=F32)
    assert torch.isfinite(E).all() and torch.isfinite(N).all()
    _check(tag + " E", E, E64, E32)
    _check(tag + " N", N, N64, N32)
    assert torch.equal(E == 0, E64 == 0), tag + ": E is zero elsewhere than the statement's"
    Ec, Nc = _nan(n, d), _nan(n, d)
    tail_fwd(ops, lib, S1, S2, b1, b2, n, d, p, stream, Ec, Nc, d)
    assert torch.equal(Ec, E) and torch.equal(Nc, N), tag + ": contiguous N and slot N have other bits"
    clamped = E64.norm(dim=1) <= 1e-12
    gE, gNfull = _randn(rng, (n, d)), _randn(rng, (n, d))
    kink = _near_the_kink(ref.tail64(S1, S2, b1, b2, 1.0, ONE())[0],
                          ref.tail64(S1.abs(), None if S2 is None else S2.abs(), b1.abs(), b2.abs(), 1.0, ONE())[0])
    gE[kink], gNfull[kink] = 0.0, 0.0
    out = {}
    for rows_name, rows in _row_sets(rng, n):
        flags = ref._flags(None if rows is None else dev(rows), n, "cuda")
        bitmap = None if rows is None else _bitmap(n, rows)
        gpanel = _nan(n, 4 * d)
        gpanel[:, 2 * d:3 * d] = torch.where(flags[:, None], gNfull, torch.full_like(gNfull, NAN))
        gN = gpanel[:, 2 * d:3 * d]
        for g_name, ge, gn in (("gE", gE, None), ("gN", None, gN), ("gE+gN", gE, gN)):
            what = "%s %s %s" % (tag, g_name, rows_name)
            gT = _nan(n, d)
            tail_bwd(ops, lib, E, ge, None if gn is None else gpanel, 4 * d, bitmap, n, d, p, stream, gT, slot=2)
            assert torch.isfinite(gT).all(), what + ": gT is not finite (NaN in memory that must not be read)"
            a = (S1, S2, b1, b2, SLOPE, mask, ge, gn, flags)
            t64, t32 = ref.tail_grads64(*a), ref.tail_grads64(*a, dtype=F32)
            hot = clamped & flags if gn is not None else torch.zeros_like(clamped)  # rows carrying the factor 1e12
            if (~hot).any() and float(t64[~hot].abs().max()) > 0 and gn is not None and d < 16:
                _check_short_rows(what + " gT", gT[~hot], t64[~hot], t32[~hot],
                                  _short_row_bound(E64, N64, mask, gn, flags, t64)[~hot])
            elif (~hot).any() and float(t64[~hot].abs().max()) > 0:
                _check(what + " gT", gT[~hot], t64[~hot], t32[~hot])
            else:
                assert (gT[~hot] == 0).all() and (t64[~hot] == 0).all()
            if hot.any() and float(t64[hot].abs().max()) > 0:
                _check(what + " gT, clamped rows", gT[hot], t64[hot], t32[hot])
            if gn is None and rows is not None:
                continue  # (gE only: the bitmap is not read; one run is enough)
            out[(g_name, rows_name)] = gT
            if gn is not None and rows is None:  # gN from a contiguous panel: same bits
                gT2 = _nan(n, d)
                tail_bwd(ops, lib, E, ge, gNfull.contiguous(), d, None, n, d, p, stream, gT2)
                assert torch.equal(gT2, gT), what + ": contiguous gN and slot gN give other bits"
    if extra is not None:
        extra(tag, E, E64, mask, gE, out)
    return clamped


@pytest.mark.parametrize("n", TAIL_N)
@pytest.mark.parametrize("d", TAIL_D)
def test_tail_vs_float64(ops, lib, d, n):
    """ngcf_tail_fwd_vec_kernel / ngcf_tail_bwd_vec_kernel<LPR> at d = 32, 64, 128, 256 (the slot pointer is 16-byte
    aligned and ldn = 4d), ngcf_tail_fwd_kernel / ngcf_tail_bwd_kernel at d = 4, 7, 48, 100 (d = 7: the slot is not
    aligned either); n = 1, 3: less than one workgroup's rows; 63 .. 65, 257: the `r >= n` exit inside a wave (vector
    forms: 64 / LPR rows per wave) and in the last workgroup; n = 65, 257: a partial last bitmap word."""
    for p in (0.0, 0.3):
        for with_s2 in (True, False):
            _tail_case(ops, lib, d, n, p, with_s2, STREAMS[0] if with_s2 else STREAMS[1])


def test_tail_fully_dropped_rows(ops, lib):
    """d = 4, p = 0.5, n = 1000 on stream (1234, 7): the 68 rows test_ngcf_ref.py counts lose all four features — E = N = 0
    (the clamp: 0 / 1e-12), and no gradient passes: gT is exactly 0 there whatever gN holds."""
    n, d = 1000, 4

    def extra(tag, E, E64, mask, gE, out):
        gone = (mask == 0).all(dim=1)
        assert int(gone.sum()) == 68
        assert (E[gone] == 0).all()
        for gT in out.values():
            assert (gT[gone] == 0).all()

    clamped = _tail_case(ops, lib, d, n, 0.5, True, STREAMS[0], key="dropped", extra=extra)
    assert int(clamped.sum()) == 68


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("d", [7, 64, 100, 256])
def test_tail_exact_zeros_of_the_preactivation(ops, lib, d, p):
    """b1 = 0.5, b2 = 0.25, S1 = -0.75 on a tenth of the elements, on all of row 3 and all of row n - 1, S2 = NULL:
    (S1 + b1) + (0 + b2) == 0.0f exactly, E = 0 there.  Rows 3 and n - 1 are clamped rows: their gT carries 1 / 1e-12 and is
    compared on its own scale (inside _tail_case).  LeakyReLU's derivative at 0: with gE alone, a kept zero element gets
    exactly (gE * keep) * slope — the kernel's own two products — and a dropped one exactly 0."""
    n = 65
    rng = _rng("zeros", d, p)
    S1 = rng.standard_normal((n, d)).astype(np.float32)
    zero = rng.random((n, d)) < 0.1
    zero[3], zero[n - 1] = True, True
    S1[zero] = -0.75
    zero = dev(zero)
    consts = (torch.full((d,), 0.5, device="cuda"), torch.full((d,), 0.25, device="cuda"), dev(S1))
    stream = STREAMS[0]

    def extra(tag, E, E64, mask, gE, out):
        assert (E[zero] == 0).all() and (E64[zero] == 0).all()
        gT = out[("gE", "all rows")]
        k32 = _mask(p, stream, n, d, dtype=F32)
        want = (gE * k32) * torch.tensor(SLOPE, dtype=F32, device="cuda")
        kept = zero & (k32 > 0)
        assert kept.any() and (want[kept] != 0).any()
        assert torch.equal(gT[kept], want[kept]), tag + ": a kept element with t == 0 does not get slope * g"
        assert (gT[zero & (k32 == 0)] == 0).all(), tag + ": a dropped element got a gradient"
        both = out[("gE+gN", "all rows")]
        assert float(both[3].abs().max()) > 1e9 and float(both[n - 1].abs().max()) > 1e9  # the clamped rows' 1 / 1e-12

    clamped = _tail_case(ops, lib, d, n, p, False, stream, key="zeros", consts=consts, extra=extra)
    assert clamped[3] and clamped[n - 1]


@pytest.mark.parametrize("d", [7, 64, 256])
def test_tail_rows_below_the_clamp_but_not_zero(ops, lib, d):
    """b = 0, S2 = NULL, rows 5 and n - 1 of S1 scaled to a norm near 2e-13 (t = S1 exactly: no sign can flip): 0 < ||E|| <
    1e-12, so N = E / 1e-12 and normalize's Jacobian is I / 1e-12 with NO projection — on an all-zero row the projection
    term vanishes by itself, here it does not (it would be a hundredth of gN).  These rows' gT on its own scale."""
    n = 65
    rng = _rng("tiny", d)
    S1 = rng.standard_normal((n, d))
    S1[5] *= 4e-13 / np.sqrt(d)
    S1[n - 1] *= 4e-13 / np.sqrt(d)
    zeros = torch.zeros(d, device="cuda")

    def extra(tag, E, E64, mask, gE, out):
        nrm = E64[[5, n - 1]].norm(dim=1)
        assert (nrm > 3e-14).all() and (nrm < 5e-13).all()
        assert float(out[("gN", "all rows")][5].abs().max()) > 1e9

    clamped = _tail_case(ops, lib, d, n, 0.0, False, STREAMS[0], key="tiny", consts=(zeros, zeros, dev(S1.astype(np.float32))),
                         extra=extra)
    assert clamped.tolist() == [r in (5, n - 1) for r in range(n)]


# ======================================================================================================== (c) the transforms
def _transform_inputs(rng, n, d1, d2):
    side, ego = _randn(rng, (n, d1), 0.5), _randn(rng, (n, d1), 0.5)
    W1, W2 = _randn(rng, (d1, d2), 0.2), _randn(rng, (d1, d2), 0.2)
    return side, ego, W1, W2


def _transform64(side, ego, W1, W2, dtype):
    side, ego = side.to(dtype), ego.to(dtype)
    return side @ W1.to(dtype) + (ego * side) @ W2.to(dtype)


def _transform_fwd_case(ops, lib, n, d1, d2):
    side, ego, W1, W2 = _transform_inputs(_rng("tf", n, d1, d2), n, d1, d2)
    S, BI = _nan(n, d2), _nan(n, d1)
    st = ops._stream()
    _ok(lib.idg_ngcf_transform_f32(_p(side), _p(ego), _p(W1), _p(W2), n, d1, d2, _p(S), _p(BI), st), "idg_ngcf_transform_f32")
    tag = "transform n=%d (%d, %d)" % (n, d1, d2)
    assert torch.isfinite(S).all()
    _check(tag + " S", S, _transform64(side, ego, W1, W2, F64), _transform64(side, ego, W1, W2, F32))
    assert torch.equal(BI, ego * side), tag + ": BI is not ego * side"
    S2 = _nan(n, d2)
    _ok(lib.idg_ngcf_transform_f32(_p(side), _p(ego), _p(W1), _p(W2), n, d1, d2, _p(S2), None, st), "idg_ngcf_transform_f32")
    assert torch.equal(S2, S), tag + ": BI = NULL changes S"


def _transform_bwd_case(ops, lib, n, d1, d2):
    rng = _rng("tb", n, d1, d2)
    side, ego, W1, W2 = _transform_inputs(rng, n, d1, d2)
    gS = _randn(rng, (n, d2))
    gs, ge = _nan(n, d1), _nan(n, d1)
    _ok(lib.idg_ngcf_transform_bwd_f32(_p(gS), _p(side), _p(ego), _p(W1), _p(W2), n, d1, d2, _p(gs), _p(ge), ops._stream()),
        "idg_ngcf_transform_bwd_f32")
    want = []
    for dtype in (F64, F32):
        a, b = (x.detach().to(dtype).clone().requires_grad_(True) for x in (side, ego))
        want.append(torch.autograd.grad(_transform64(a, b, W1, W2, dtype), (a, b), grad_outputs=gS.to(dtype)))
    tag = "transform' n=%d (%d, %d)" % (n, d1, d2)
    assert torch.isfinite(gs).all() and torch.isfinite(ge).all()
    _check(tag + " g_side", gs, want[0][0], want[1][0])
    _check(tag + " g_ego", ge, want[0][1], want[1][1])


TRANSFORM_N = [1, 31, 32, 33, 257]
BIG_N = 24577 + 5  # 769 row tiles: past the 768 a full grid of 3072 waves covers at four column tiles


@pytest.mark.parametrize("n", TRANSFORM_N)
@pytest.mark.parametrize("d1,d2", [(64, 32), (64, 96), (64, 64), (128, 64), (128, 128), (192, 64)])
def test_transform_forward_vs_float64(ops, lib, d1, d2, n):
    """d2 = 32, 96: one and three column tiles (the grid's multiple of nct * 4 waves); d1 = 128, 192: the second and third
    64-chunk's read-modify-write of S; n < 32 and n = 33: rows past the end clamp to the last row; every n here is fewer
    tasks than the grid's minimum of nct * 4 waves or just above it."""
    _transform_fwd_case(ops, lib, n, d1, d2)


@pytest.mark.parametrize("n", TRANSFORM_N)
@pytest.mark.parametrize("d1,d2", [(32, 64), (96, 64), (64, 64), (64, 128), (128, 192)])
def test_transform_backward_vs_float64(ops, lib, d1, d2, n):
    """d2 = 64: the weights kept in registers; d2 = 128, 192: the chunk loop; d1 = 32, 96: one and three feature tiles."""
    _transform_bwd_case(ops, lib, n, d1, d2)


def test_transform_persistent_walk_past_one_tile_per_wave(ops, lib):
    """n = 24,582 with four tiles across (d2 = 128 forward, d1 = 128 backward): 3076 tasks on the full grid of 3072 waves —
    wave 0 .. 3 walk a second row tile, which is also the partial last one."""
    _transform_fwd_case(ops, lib, BIG_N, 128, 128)
    _transform_bwd_case(ops, lib, BIG_N, 128, 192)


def test_transform_refused_widths_write_nothing(ops, lib):
    n = 40
    st = ops._stream()
    side, ego, W = torch.ones(n, 64, device="cuda"), torch.ones(n, 64, device="cuda"), torch.ones(64, 64, device="cuda")
    S, BI, gs, ge = (torch.full((n, 64), 7.0, device="cuda") for _ in range(4))
    assert lib.idg_ngcf_transform_f32(_p(side), _p(ego), _p(W), _p(W), n, 48, 64, _p(S), _p(BI), st) != 0
    assert lib.idg_ngcf_transform_bwd_f32(_p(S), _p(side), _p(ego), _p(W), _p(W), n, 64, 32, _p(gs), _p(ge), st) != 0
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in (S, BI, gs, ge))
    assert lib.idg_ngcf_transform_f32(_p(side), _p(ego), _p(W), _p(W), n, 64, 64, _p(S), _p(BI), st) == 0


# ================================================================================================================= (d) wgrad
def _blocks(d1, d2):
    ww = d1 * d2
    return (("g W1", 0, ww), ("g b1", ww, ww + d2), ("g W2", ww + d2, 2 * ww + d2), ("g b2", 2 * ww + d2, 2 * ww + 2 * d2))


def _wgrad64(side, bi, gT, dtype):
    s, b, t = side.to(dtype), bi.to(dtype), gT.to(dtype)
    return torch.cat([(s.t() @ t).reshape(-1), t.sum(0), (b.t() @ t).reshape(-1), t.sum(0)])


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513])
@pytest.mark.parametrize("d1,d2", [(64, 64), (128, 64), (64, 128)])
def test_wgrad_vs_float64(ops, lib, d1, d2, n):
    """slices = min(n, 512): one row per slice up to n = 512, then ceil(n / 512) = 2 rows on the first 257 slices and none
    on the rest (n = 513).  The workspace holds NaN before each call: every slice that is summed was written."""
    rng = _rng("wgrad", n, d1, d2)
    side, bi, gT = _randn(rng, (n, d1), 0.5), _randn(rng, (n, d1), 0.5), _randn(rng, (n, d2))
    ws = torch.empty(int(lib.idg_ngcf_wgrad_workspace_bytes(d1, d2)) // 4, device="cuda")
    outs = []
    for _ in range(2):
        ws.fill_(NAN)
        out = _nan(2 * d1 * d2 + 2 * d2)
        _ok(lib.idg_ngcf_wgrad_f32(_p(side), _p(bi), _p(gT), n, d1, d2, _p(out), _p(ws), ops._stream()), "idg_ngcf_wgrad_f32")
        outs.append(out)
    assert torch.isfinite(outs[0]).all()
    w64, w32 = _wgrad64(side, bi, gT, F64), _wgrad64(side, bi, gT, F32)
    for name, lo, hi in _blocks(d1, d2):
        _check("wgrad n=%d (%d, %d) %s" % (n, d1, d2, name), outs[0][lo:hi], w64[lo:hi], w32[lo:hi])
    assert torch.equal(outs[0], outs[1]), "the second call gave other bits"


# ================================================================================================ (e) the fused layer kernels
LAYER_N = [1, 63, 64, 65, 129, 4133, 512 * 64 + 65]


def _layer_case(ops, lib, n, p, key="layer", zero_row=None, tiny=False):
    """Forward (N into slot 2 of a [n, 256] panel) and the backward for gE / gN / both times the three row sets: the band
    rule on E, N, g_side, g_ego and the four parameter gradients, and bit equality with the chain of idg_dense.hip."""
    d, D = 64, 256
    rng = _rng(key, n, p)
    stream = STREAMS[1] if n % 2 else STREAMS[0]
    side, ego = _randn(rng, (n, d), 0.3), _randn(rng, (n, d), 0.3)
    W1, W2 = _randn(rng, (d, d), 0.1), _randn(rng, (d, d), 0.1)
    b1, b2 = _randn(rng, (d,), 0.1), _randn(rng, (d,), 0.1)
    if tiny:
        side[zero_row] *= 1e-13
        b1, b2 = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    elif zero_row is not None:
        side[zero_row] = 0.0
        b1, b2 = torch.full((d,), 0.5, device="cuda"), torch.full((d,), -0.5, device="cuda")
    mask = _mask(p, stream, n, d)
    tag = "%s n=%d p=%g" % (key, n, p)
    st = ops._stream()
    E, panel = _nan(n, d), torch.full((n, D), 7.0, device="cuda")
    _ok(lib.idg_ngcf_layer_fwd_f32(_p(side), _p(ego), _p(W1), _p(W2), _p(b1), _p(b2), n, d, SLOPE, p, stream[0], stream[1], _p(E),
                                   _p(panel, 2 * d), D, st), "idg_ngcf_layer_fwd_f32")
    assert (panel[:, :2 * d] == 7.0).all() and (panel[:, 3 * d:] == 7.0).all(), tag + ": the panel was written outside the slot"
    N = panel[:, 2 * d:3 * d]
    E64, N64 = ref.layer64(side, ego, W1, W2, b1, b2, SLOPE, mask)
    E32, N32 = ref.layer64(side, ego, W1, W2, b1, b2, SLOPE, mask, dtype=F32)
    assert torch.isfinite(E).all() and torch.isfinite(N).all()
    _check(tag + " E", E, E64, E32)
    _check(tag + " N", N, N64, N32)
    # the chain
    S, BI, Ec, Nc = _nan(n, d), _nan(n, d), _nan(n, d), _nan(n, d)
    _ok(lib.idg_ngcf_transform_f32(_p(side), _p(ego), _p(W1), _p(W2), n, d, d, _p(S), _p(BI), st), "idg_ngcf_transform_f32")
    tail_fwd(ops, lib, S, None, b1, b2, n, d, p, stream, Ec, Nc, d)
    assert torch.equal(Ec, E) and torch.equal(Nc, N), tag + ": the fused forward and the chain differ"
    if tiny:
        assert 1e-14 < float(E64[zero_row].norm()) < 5e-13 and float(E[zero_row].abs().max()) > 0
    elif zero_row is not None:
        assert (E[zero_row] == 0).all() and (N[zero_row] == 0).all()
    clamped = E64.norm(dim=1) <= 1e-12
    gE, gNfull = _randn(rng, (n, d)), _randn(rng, (n, d))
    kink = _near_the_kink(ref.layer64(side, ego, W1, W2, b1, b2, 1.0, ONE())[0],
                          ref.layer64(side.abs(), ego.abs(), W1.abs(), W2.abs(), b1.abs(), b2.abs(), 1.0, ONE())[0])
    print("  %s: %d rows next to the kink carry no upstream gradient" % (tag, int(kink.sum())))
    gE[kink], gNfull[kink] = 0.0, 0.0
    ws = torch.empty(int(lib.idg_ngcf_layer_bwd_workspace_bytes(d)) // 4, device="cuda")
    row_sets = _row_sets(rng, n)
    if zero_row is not None:
        row_sets[1] = ("5% of rows", np.unique(np.append(row_sets[1][1], zero_row)))
    for rows_name, rows in row_sets:
        flags = ref._flags(None if rows is None else dev(rows), n, "cuda")
        bitmap = None if rows is None else _bitmap(n, rows)
        gpanel = _nan(n, D)
        gpanel[:, 2 * d:3 * d] = torch.where(flags[:, None], gNfull, torch.full_like(gNfull, NAN))
        for g_name, ge, use_gn in (("gE", gE, False), ("gN", None, True), ("gE+gN", gE, True)):
            if not use_gn and rows is not None:
                continue
            what = "%s %s %s" % (tag, g_name, rows_name)
            gs, gg, wg = _nan(n, d), _nan(n, d), _nan(2 * d * d + 2 * d)
            ws.fill_(NAN)
            _ok(lib.idg_ngcf_layer_bwd_f32(_p(E), _p(ge), _p(gpanel, 2 * d) if use_gn else None, D, _p(bitmap), _p(side), _p(ego),
                                           _p(W1), _p(W2), n, d, SLOPE, p, stream[0], stream[1], _p(gs), _p(gg), _p(wg), _p(ws),
                                           st), "idg_ngcf_layer_bwd_f32")
            assert torch.isfinite(gs).all() and torch.isfinite(gg).all(), what + ": NaN from memory that must not be read"
            assert torch.isfinite(wg).all(), what + ": a workspace slice was summed but never written"
            gn = gpanel[:, 2 * d:3 * d] if use_gn else None
            a = (side, ego, W1, W2, b1, b2, SLOPE, mask, ge, gn, flags)
            r64, r32 = ref.layer_grads64(*a), ref.layer_grads64(*a, dtype=F32)
            hot = clamped & flags if use_gn else torch.zeros_like(clamped)
            for k, (name, got) in enumerate((("g_side", gs), ("g_ego", gg)), 1):
                _check("%s %s" % (what, name), got[~hot], r64[k][~hot], r32[k][~hot])
                if hot.any() and float(r64[k][hot].abs().max()) > 0:
                    _check("%s %s, clamped rows" % (what, name), got[hot], r64[k][hot], r32[k][hot])
                elif hot.any():
                    assert (got[hot] == 0).all()
            for name, lo, hi in _blocks(d, d):
                _check("%s %s" % (what, name), wg[lo:hi], r64[3][lo:hi], r32[3][lo:hi])
            # the chain: tail' + transform'
            gT, gs0, gg0 = _nan(n, d), _nan(n, d), _nan(n, d)
            tail_bwd(ops, lib, E, ge, gpanel if use_gn else None, D, bitmap, n, d, p, stream, gT, slot=2)
            _ok(lib.idg_ngcf_transform_bwd_f32(_p(gT), _p(side), _p(ego), _p(W1), _p(W2), n, d, d, _p(gs0), _p(gg0), st),
                "idg_ngcf_transform_bwd_f32")
            assert torch.equal(gs0, gs) and torch.equal(gg0, gg), what + ": the fused backward and the chain differ"
            wg2 = _nan(2 * d * d + 2 * d)
            ws.fill_(NAN)
            _ok(lib.idg_ngcf_layer_bwd_f32(_p(E), _p(ge), _p(gpanel, 2 * d) if use_gn else None, D, _p(bitmap), _p(side), _p(ego),
                                           _p(W1), _p(W2), n, d, SLOPE, p, stream[0], stream[1], _p(gs0), _p(gg0), _p(wg2), _p(ws),
                                           st), "idg_ngcf_layer_bwd_f32")
            assert torch.equal(wg2, wg), what + ": the second call gave other parameter gradients"


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("n", LAYER_N)
def test_fused_layer_kernels_vs_float64_and_the_chain(ops, lib, n, p):
    """n <= 64: one workgroup, one slice; n = 65, 129: 2 and 3 workgroups, the last with one live row; 4133: 65 slices, the
    reduction's second group of 16; 512 * 64 + 65 = 32,833 rows: 515 blocks on 512 persistent workgroups — the first three
    walk a second block."""
    _layer_case(ops, lib, n, p)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_fused_layer_kernels_on_a_clamped_row(ops, lib, p):
    """side row = 0 with b1 = 0.5, b2 = -0.5: t = (0 + 0.5) + (0 - 0.5) = 0 on the whole row, E = 0, the row is clamped and
    its gT = slope * keep * (gE + gN / 1e-12): g_side of that row on its own scale, g_ego exactly 0 (side = 0); the bias
    gradients take the row's 1e12-sized terms on THEIR scale."""
    _layer_case(ops, lib, 129, p, key="layer-zero-row", zero_row=70)


def test_fused_layer_kernels_on_a_row_below_the_clamp_but_not_zero(ops, lib):
    """side row scaled by 1e-13 with b = 0: 0 < ||E|| < 1e-12 — the clamp branch with E != 0, where keeping the projection
    would show (see test_tail_rows_below_the_clamp_but_not_zero)."""
    _layer_case(ops, lib, 129, 0.0, key="layer-tiny-row", zero_row=70, tiny=True)


# ================================================================================================================ (f) the engine
N_USERS, N_ITEMS = 150, 107
REG, LR = float(np.float32(1e-4)), 1e-3
ENGINE_CASES = [(64, 3, 256, 0.1, "1"), (64, 1, 1, 0.0, "1"), (64, 2, 97, 0.5, "0"), (128, 3, 256, 0.1, "1"),
                (128, 1, 97, 0.0, "1"), (256, 2, 256, 0.1, "1")]
_engine_runs = {}
_graphs = {}


def _graph(ops):
    """A random symmetric user-item graph with self loops, D^-1/2 (A + I) D^-1/2 (data_graph.sparse_adjacency_matrix_with_self),
    n = 257 rows; one user with 60 items, one item with 70 users, one user and one item with no edge but the self loop."""
    if "g" not in _graphs:
        import scipy.sparse as sp

        rng = _rng("graph")
        M = rng.random((N_USERS, N_ITEMS)) < 0.05
        M[5, rng.choice(N_ITEMS, 60, replace=False)] = True
        M[rng.choice(N_USERS, 70, replace=False), 9] = True
        M[17, :] = False
        M[:, 23] = False
        n = N_USERS + N_ITEMS
        A = np.zeros((n, n), dtype=bool)
        A[:N_USERS, N_USERS:], A[N_USERS:, :N_USERS] = M, M.T
        A |= np.eye(n, dtype=bool)
        deg = A.sum(axis=1).astype(np.float64)
        vals = (1.0 / np.sqrt(np.outer(deg, deg)))[A]
        m = sp.csr_matrix((vals.astype(np.float32), np.nonzero(A)), shape=(n, n))
        m.sort_indices()
        assert (m != m.T).nnz == 0
        _graphs["g"] = (ops.Graph(m.indptr, m.indices, m.data, n, n),
                        ref.dense_operator(m.indptr, m.indices, m.data, (n, n), device="cuda"))
    return _graphs["g"]


def _batch(rng, B):
    users, pos, neg = rng.integers(0, N_USERS, B), rng.integers(0, N_ITEMS, B), rng.integers(0, N_ITEMS, B)
    if B >= 70:
        q = rng.choice(B, 70, replace=False)
        pos[q] = pos[q[0]]
    return tuple(dev(x.astype(np.int64)) for x in (users, pos, neg))


def _engine_run(ops, monkeypatch, d, K, B, p, layer_env):
    """Two training steps with store_grad and known dropout streams, every step next to step64 in float64 and float32 FROM
    THE ENGINE'S OWN TABLES read back before the step; then the same two steps without store_grad."""
    key = (d, K, B, p, layer_env)
    if key in _engine_runs:
        return _engine_runs[key]
    from idgrec_amd.ngcf import NgcfEngine

    monkeypatch.setenv("IDG_NGCF_LAYER", layer_env)
    G, A64 = _graph(ops)
    n = N_USERS + N_ITEMS
    rng = _rng("engine", *key)
    xav = lambda r, c: dev(rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32))  # noqa: E731
    P0 = torch.cat([xav(N_USERS, d), xav(N_ITEMS, d)])
    small0 = [(xav(d, d), xav(1, d), xav(d, d), xav(1, d)) for _ in range(K)]
    batches = [_batch(rng, B), _batch(rng, B)]
    seeds = [STREAMS[1][0], 77]

    def make(store_grad):
        eng = NgcfEngine(G, N_USERS, N_ITEMS, P0.clone(), small0, slope=0.2, mess_dropout=[p] * K, reg_lambda=REG, lr=LR,
                         store_grad=store_grad)
        assert eng.fused_layer == (d == 64 and layer_env == "1")
        return eng

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
            masks = [_mask(p, sd, n, d, dtype=dtype) for sd in streams]
            losses, gE0, gsmall, final = ref.step64(A64, P_before, small_before, users, pos, neg, SLOPE, masks, REG, N_USERS,
                                                    dtype=dtype)
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


@pytest.mark.parametrize("d,K,B,p,layer_env", ENGINE_CASES)
def test_engine_two_steps_vs_float64(ops, monkeypatch, d, K, B, p, layer_env):
    """d = 64: the fused layer kernels, and with IDG_NGCF_LAYER=0 the chain; d = 128, 256: the chain — transform, tail into
    the panel's slot, tail' with the batch's bitmap and ldgn = (K + 1) d, idg_ngcf_wgrad_f32, transform'."""
    run = _engine_run(ops, monkeypatch, d, K, B, p, layer_env)
    per = 2 * d * d + 2 * d
    for s, st in enumerate(run["steps"], 1):
        tag = "engine d=%d K=%d B=%d p=%g %s step %d" % (d, K, B, p, "fused" if (d == 64 and layer_env == "1") else "chain", s)
        assert torch.isfinite(st["loss"]).all() and torch.isfinite(st["GRAD"]).all() and torch.isfinite(st["SG"]).all()
        for k, name in enumerate(("bpr", "reg")):
            _check("%s loss %s" % (tag, name), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " final", st["final"], st["final64"], st["final32"])
        _check(tag + " GRAD", st["GRAD"], st["GRAD64"], st["GRAD32"])
        for l in range(K):
            for name, lo, hi in _blocks(d, d):
                lo, hi = l * per + lo, l * per + hi
                _check("%s layer %d %s" % (tag, l, name), st["SG"][lo:hi], st["SG64"][lo:hi], st["SG32"][lo:hi])


@pytest.mark.parametrize("d,K,B,p,layer_env", ENGINE_CASES)
def test_engine_adam_state_after_each_step(ops, monkeypatch, d, K, B, p, layer_env):
    """The rule of test_gpu_egcf.py::test_engine_adam_state_after_each_step, on the embedding panel (Adam in the last
    product's epilogue) and on the flat buffer of the 4K small tensors (one launch): exp_avg, exp_avg_sq within 4 * 2^-24
    of their largest entry, the parameters within 4 ulp of their largest entry, against the float64 recurrence fed the
    engine's own two gradients from the float32 initial values."""
    run = _engine_run(ops, monkeypatch, d, K, B, p, layer_env)
    for what, W0, gk, wk, mk, vk in (("panel", run["P0"], "GRAD", "P", "M", "V"), ("small", run["SW0"], "SG", "SW", "SM", "SV")):
        want = ref.adam64(W0, [st[gk] for st in run["steps"]], lr=LR)
        for s, (st, (W, M, V)) in enumerate(zip(run["steps"], want), 1):
            for name, got, w in (("exp_avg", st[mk], M), ("exp_avg_sq", st[vk], V)):
                e = float((got.double() - w).abs().max() / w.abs().max())
                print("  d=%d K=%d %s step %d %s: %.2f * 2^-24 of max" % (d, K, what, s, name, e * 2.0 ** 24))
                assert e <= 4 * 2.0 ** -24, (what, name, s, e)
            wmax = float(W.abs().max())
            ulp = float(np.spacing(np.float32(wmax)))
            e = float((st[wk].double() - W).abs().max())
            print("  d=%d K=%d %s step %d parameters: %.2f ulp of max |W| = %.3f" % (d, K, what, s, e / ulp, wmax))
            assert e <= 4 * ulp, (what, s, e / ulp)
        assert not torch.equal(run["steps"][0][wk], run["steps"][1][wk])


@pytest.mark.parametrize("d,K,B,p,layer_env", ENGINE_CASES)
def test_engine_without_stored_gradient_is_bit_identical(ops, monkeypatch, d, K, B, p, layer_env):
    run = _engine_run(ops, monkeypatch, d, K, B, p, layer_env)
    last = run["steps"][-1]
    for got, name in zip(run["lean"], ("P", "M", "V", "SW", "SM", "SV")):
        assert torch.equal(got, last[name]), name
