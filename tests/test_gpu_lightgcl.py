"""LightGCL's kernels (idgrec_amd/csrc/idg_svdnce.hip), their operators (ops.lowrank_project, ops.lowrank_expand,
ops.svd_nce_loss), the engine (idgrec_amd/lightgcl.py) and the plugin (models/LightGCL.py) on the device.  The reference
statement is tests/lightgcl_ref64.py, pinned to the reference's own float64 run by tests/test_lightgcl_host.py; nothing here is
measured against the code under test.

  (a) idg_svd_nce_f32, both losses and all four gradient outputs, against float64 over a pruned grid in which every value of
      d in {32, 48, 64, 256}, B in {1, 127, 129, 300}, N in {1, 127, 128, 129, 1000}, q in {1, 5, 16}, both sides (row0 = 0 and
      row0 > 0), tau in {0.2, 1.0} appears; ids with repeats, and one id filling the whole batch;
      and, on the matrix-core passes (B = 129 and 300), the widths of tests/widths.py (EVERY_NDT, LIGHTGCL_CHUNKED), which
      launch svd_tile_kernel at every NDT = ceil(d / 32) = 1 .. 8 in its three modes (the loss-only call included; d = 128
      with gradients is the one form of NDT <= 4 that takes a whole CU per workgroup);
  (b) the clamp: about half of the rows outside [-5, 5] on either end, none within 1e-3 of the kink; a clamped row's positive
      term has EXACTLY zero gradient;
  (c) scores near 200 (where the reference's exp overflows fp32): finite loss within tolerance, finite gradients; and scores
      far below zero, where the 1e-8 is the whole sum;
  (d) the accumulation contract (pre-filled panels come back as pattern + gradient, every other row bit-unchanged, dP stored),
      identical bits on a second run and from the loss-only call;
  (e) the projection and the expansion: n in {1, 255, 4097}, q in {1, 5, 16}, d in {32, 48, 256}, row strides wider than the
      rows, the row-id form with repeats, the accumulate and scale arguments, and both under autograd;
  (f) ops.svd_nce_loss under autograd is the raw call;
  (g) LightgclEngine from the fixture's tables, batches and factors, both settings: three fused steps against the fixture's
      losses and the float64 trajectory, the fused step against forward() + autograd + ops.Adam, and K = 1;
  (h) the plugin: one epoch through the trainer on a generated dataset, get_rating_for_test against float64 rows.

Tolerances.  Every kernel comparison measures, in the same test, how far the plain float32 torch composition of the
reference's expressions (tests/lightgcl_ref64.py with dtype = float32, on the CPU) lies from the float64 statement, relative
to the largest entry of the compared array, and allows the kernel TWICE that: both are fp32 evaluations with different
summation orders.  The yardstick is itself quantised — on a one-row table the float32 composition can round to the float64
value exactly — so the allowance never goes below 2^-23 of the largest entry: a correctly rounded fp32 result is half a unit
in the last place from the exact one, and twice that is one unit.  A loss is the mean of B per-row terms, and the clamped
positives have both signs and cancel (a mean of -0.012 from terms of size 5): its "largest entry" is the largest per-row
term, which is what its rounding scales with, not the mean.  Where the reference's own expression overflows in float32
(case c) the yardstick is the running-maximum form in float32.  The engine's losses take rtol 1e-5 and its three-step tables
the criterion tests/test_gpu_mixrec.py applies to the same comparison (under 1e-3 of the elements outside rtol 1e-4 / atol
1e-6, none further than 1e-4); its gradient takes twice the float32 layered composition's distance on the fixture's inputs.

Measured on an MI355X (34 tests, 31 s for the whole file, 26 s of it the first import).  (a) gradients 0.6e-7 .. 1.4e-6 of the
largest entry where float32 torch sits 0.6e-7 .. 1.5e-6 (0.3 .. 1.1 of it), losses 0.6e-7 .. 2.4e-6 absolute; (b) (c) below the
yardstick itself; (g) the fused step's gradient 6.4e-8 (`def`), 3.3e-7 (`clamp`), 1.1e-7 (K = 1) of the largest entry against
bounds of 3.1e-7, 5.4e-7, 2.0e-7, tables within 9.1e-7 of float64 after every step.
Batches below one tile (B <= 127) take the kernel's direct form, whose scores and weights are double: at B = 1 (N = 129,
d = 48) g_final sits 5.1e-8 of the largest entry from float64, float32 torch 5.1e-8 — what is left is the fp32 rounding of
the view row itself.  (Through the matrix-core passes the same case sat at 2.6e-7, bound 1.2e-7: with one batch row nothing
averages, and a weight carries the fp32 rounding of two dot products that 1 / tau multiplies.)  B = 127 and B = 128 are the
two sides of that threshold; the engine tests run both forms (B = 96 and B = 128 batches).
With the cases over every built width (48 tests, 5 s without the first import; the 14 new cases under 0.2 s together):
gradients 1.2e-7 .. 3.1e-6 of the largest entry where float32 torch sits 2.1e-7 .. 3.1e-6, at most 0.69 of the bound (g_ego at
d = 32); losses within 1.0e-7 absolute (0.26 of the bound); the loss-only call's bits equal at every NDT.  (When these cases
first ran, the tile passes added a score's d features in one fp32 chain: g_ego at d = 224, B = N = 129, tau = 0.2 sat 3.69e-6 of
the largest entry from float64 — float32 torch 1.61e-6, bound 3.21e-6 — and failed, with d = 160 and d = 200 at 0.98 of their
bounds.  The scores are now summed 32 features at a time, csrc/idg_svdnce.hip: score_tile_chunked; the same case sits at
6.6e-7, d = 160 and d = 200 at 0.30 and 0.55 of their bounds at most.)"""
import importlib
import io
import logging
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import lightgcl_ref64 as ref  # noqa: E402
from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23
LOSS_RTOL = 1e-5
PARAMS = ("user_embedding", "item_embedding")


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


def _gen(*key):
    import zlib

    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rel(a, want):
    """Largest difference relative to the largest entry of `want` (1 when `want` is all zero and `a` is not)."""
    scale = float(want.abs().max())
    diff = float((a.double() - want.double()).abs().max())
    return diff / scale if scale > 0 else (0.0 if diff == 0 else 1.0)


# ================================================================================================== (a) the kernel vs float64
def _case(key, d, B, N, q, row0, ids="random", scale=0.35):
    """(final panel, ego panel [row0 + N + 11, d], AS [N, q], P [q, d], ids [B]) float32 on the CPU."""
    gen = _gen(key, d, B, N, q, row0)
    n = row0 + N + 11
    Fp = torch.randn(n, d, generator=gen) * scale
    Ep = torch.randn(n, d, generator=gen) * scale
    AS = torch.randn(N, q, generator=gen) * 0.5
    P = torch.randn(q, d, generator=gen) * scale
    if ids == "same":
        idv = torch.full((B,), N // 2, dtype=torch.int64)
    else:
        idv = torch.randint(0, N, (B,), generator=gen)
        if B >= 3:
            idv[B - 1] = idv[0]  # a repeat, whatever the draw
    return Fp, Ep, AS, P, idv


def _run(ops, Fp, Ep, row0, N, AS, P, ids, tau, upstream=None, base=None, grads=True):
    """The raw call on the device: (loss [2], gF, gE, dP) on the CPU (None without gradients)."""
    dv = lambda t: None if t is None else t.cuda().contiguous()  # noqa: E731
    loss = torch.full((2,), float("nan"), device="cuda")
    if not grads:
        ops.svd_nce_raw(dv(Fp), dv(Ep), row0, N, dv(AS), dv(P), dv(ids), tau, loss=loss)
        return loss.cpu(), None, None, None
    gF = torch.zeros_like(Fp).cuda() if base is None else dv(base[0])
    gE = torch.zeros_like(Ep).cuda() if base is None else dv(base[1])
    dP = torch.full_like(P, float("nan")).cuda()
    up = None if upstream is None else torch.tensor(upstream, dtype=F32, device="cuda")
    ops.svd_nce_raw(dv(Fp), dv(Ep), row0, N, dv(AS), dv(P), dv(ids), tau, loss=loss, upstream=up, g_final=gF, g_ego=gE, dP=dP)
    torch.cuda.synchronize()
    return loss.cpu(), gF.cpu(), gE.cpu(), dP.cpu()


def _check(tag, ops, Fp, Ep, row0, N, AS, P, ids, tau, upstream=(1.0, 1.0), naive32=True):
    # the statements take what the kernel is handed: tau and the upstream pair as the float32 values the call carries
    tau, upstream = float(np.float32(tau)), tuple(float(np.float32(u)) for u in upstream)
    want = ref.svd_nce64(Fp, Ep, row0, N, AS, P, ids, tau, upstream=upstream)
    yard = ref.svd_nce64(Fp, Ep, row0, N, AS, P, ids, tau, upstream=upstream, dtype=F32, naive=naive32)
    got = _run(ops, Fp, Ep, row0, N, AS, P, ids, tau, upstream=upstream)
    worst = 0.0
    for k, name in enumerate(("log-sum-exp term", "clamped positive term")):
        e = abs(float(got[0][k]) - float(want[0][k]))
        tol = max(2 * abs(float(yard[0][k]) - float(want[0][k])), ULP * float(want[5][k].abs().max()))
        print("  %-58s %-22s %.3e (float32 torch %.3e, bound %.3e)" % (tag, name, e, abs(float(yard[0][k]) - float(want[0][k])), tol))
        assert np.isfinite(float(got[0][k])) and e <= tol, (tag, name, e, tol)
    for k, name in ((1, "g_final"), (2, "g_ego"), (3, "dP")):
        e, y = _rel(got[k], want[k]), _rel(yard[k], want[k])
        tol = max(2 * y, ULP)
        worst = max(worst, e / tol)
        print("  %-58s %-22s %.3e of the largest entry (float32 torch %.3e, bound %.3e)" % (tag, name, e, y, tol))
        assert torch.isfinite(got[k]).all() and e <= tol, (tag, name, e, tol)
    return got, want


GRID = [  # d, B, N, q, row0, tau, ids
    (32, 1, 1, 1, 0, 0.2, "random"),
    (48, 127, 127, 5, 37, 1.0, "random"),
    (64, 129, 128, 16, 0, 0.2, "random"),
    (256, 300, 129, 5, 37, 0.2, "random"),
    (64, 300, 1000, 5, 0, 1.0, "random"),
    (32, 129, 1000, 16, 37, 0.2, "same"),
    (48, 1, 129, 1, 0, 0.2, "random"),
    (64, 127, 1, 5, 37, 1.0, "random"),
    (256, 129, 127, 1, 0, 1.0, "same"),
    (64, 128, 129, 5, 0, 0.2, "random"),  # the first batch size on the matrix-core passes (below it: the direct form)
]


@pytest.mark.parametrize("d,B,N,q,row0,tau,ids", GRID)
def test_kernel_vs_float64_over_the_dispatch(ops, d, B, N, q, row0, tau, ids):
    Fp, Ep, AS, P, idv = _case("grid", d, B, N, q, row0, ids)
    if B >= 3:
        assert len(set(idv.tolist())) < B
    _check("d=%d B=%d N=%d q=%d row0=%d tau=%g %s" % (d, B, N, q, row0, tau, ids), ops, Fp, Ep, row0, N, AS, P, idv, tau,
           upstream=(0.7, -1.3))


def _width_id(d, B, grads="gradients"):
    one = "-one-workgroup-per-CU" if d == 128 else ""  # <4, MODE_SUMS_ACC>: the source's own launch-bounds exception
    return "d%d-NDT%d-B%d-%s%s" % (d, widths.ndt(d), B, grads, one)


# every NDT = ceil(d / 32) of svd_tile_kernel, all above SMALL_B (the matrix-core passes): d, B, N, q, row0, tau, ids
WIDTH_GRID = [pytest.param(d, 129, 129, 5, 37, 0.2, "random", id=_width_id(d, 129)) for d in widths.EVERY_NDT] \
    + [pytest.param(d, 300, 1000, 16, 0, 1.0, "same", id=_width_id(d, 300)) for d in widths.LIGHTGCL_CHUNKED]  # table chunks, query splits


@pytest.mark.parametrize("d,B,N,q,row0,tau,ids", WIDTH_GRID)
def test_kernel_vs_float64_over_every_built_width(ops, d, B, N, q, row0, tau, ids):
    """<NDT, MODE_SUMS_ACC> and <NDT, MODE_TABLE> with gradients; at B = 129 the loss-only call too (<NDT, MODE_SUMS>), which
    gives the bits of the gradient call's loss."""
    assert B > 127
    Fp, Ep, AS, P, idv = _case("widths", d, B, N, q, row0, ids)
    assert len(set(idv.tolist())) < B
    got, _ = _check("d=%d (NDT %d) B=%d N=%d q=%d row0=%d tau=%g %s" % (d, widths.ndt(d), B, N, q, row0, tau, ids), ops, Fp, Ep, row0,
                    N, AS, P, idv, tau, upstream=(0.7, -1.3))
    if B == 129:
        alone = _run(ops, Fp, Ep, row0, N, AS, P, idv, float(np.float32(tau)), grads=False)
        assert torch.equal(alone[0].view(torch.int32), got[0].view(torch.int32)), "the loss-only call gives other bits"


# ================================================================================================================ (b) the clamp
@pytest.mark.parametrize("row0", [0, 37])
def test_clamp_zeroes_the_positive_gradient_exactly(ops, row0):
    d, B, N, q, tau = 64, 129, 200, 5, 0.2
    Fp, Ep, AS, P, idv = _case("clamp", d, B, N, q, row0, scale=0.42)
    pos = ref.svd_nce64(Fp, Ep, row0, N, AS, P, idv, tau)[4]
    outside = pos.abs() > 5
    share = float(outside.double().mean())
    assert 0.3 <= share <= 0.7, share
    assert float((pos > 5).double().mean()) > 0.1 and float((pos < -5).double().mean()) > 0.1  # both ends
    assert float((pos.abs() - 5).abs().min()) > 1e-3
    _check("clamp row0=%d (%.0f %% of the rows outside)" % (row0, 100 * share), ops, Fp, Ep, row0, N, AS, P, idv, tau)
    # the positive term alone: rows whose every occurrence clamps receive exactly nothing, the others something
    loss, gF, gE, dP = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau, upstream=(0.0, 1.0))
    dead = torch.ones(N, dtype=torch.bool)
    dead[idv[~outside]] = False
    assert int(dead[idv].sum()) > 0
    assert float(gF[row0:row0 + N][dead].abs().max()) == 0 and float(gE[row0:row0 + N][dead].abs().max()) == 0
    live = torch.unique(idv[~outside])
    assert float(gE[row0:row0 + N][live].abs().max(dim=1).values.min()) > 0
    want = ref.svd_nce64(Fp, Ep, row0, N, AS, P, idv, tau, upstream=(0.0, 1.0))
    assert abs(float(loss[1]) - float(want[0][1])) <= 1e-6 * abs(float(want[0][1]))


# ======================================================================================================= (c) large and tiny scores
def test_scores_near_200_stay_finite_and_correct(ops):
    d, B, N, q, row0, tau = 64, 129, 300, 5, 0, 0.2
    Fp, Ep, AS, P, idv = _case("large", d, B, N, q, row0)
    s = (Ep[idv] + AS[idv] @ P).double() @ Fp[:N].double().t() / tau
    k = (200.0 / float(s.max())) ** 0.5
    Fp, Ep, P = Fp * k, Ep * k, P * k
    s = (Ep[idv] + AS[idv] @ P).double() @ Fp[:N].double().t() / tau
    assert 190 < float(s.max()) < 210
    naive = torch.log(torch.exp(s.float()).sum(1) + 1e-8)
    assert not torch.isfinite(naive).all()  # the reference's expression overflows in float32 here
    got, want = _check("max score %.0f" % float(s.max()), ops, Fp, Ep, row0, N, AS, P, idv, tau, naive32=False)
    assert float(want[0][0]) > 20 and all(torch.isfinite(t).all() for t in got)


def test_scores_far_below_zero_keep_the_guard(ops):
    """Every score near -60: sum_j exp(s) is far below 1e-8 and the term is log(1e-8) to float32 — a bound on the scores'
    size in place of their maximum would overflow or lose this."""
    d, B, N, q, tau = 32, 127, 130, 1, 0.2
    gen = _gen("tiny")
    Fp = torch.rand(N + 11, d, generator=gen) * 0.2 + 0.5
    Ep = -(torch.rand(N + 11, d, generator=gen) * 0.2 + 0.95)
    AS, P = torch.zeros(N, q), torch.zeros(q, d)
    idv = torch.randint(0, N, (B,), generator=gen)
    s = Ep[idv].double() @ Fp[:N].double().t() / tau
    assert float(s.max()) < -50
    got, want = _check("all scores below %.0f" % float(s.max()), ops, Fp, Ep, 0, N, AS, P, idv, tau)
    assert abs(float(want[0][0]) - np.log(1e-8)) < 1e-6 and abs(float(got[0][0]) - np.log(1e-8)) < 1e-5


# ============================================================================ (d) accumulation, untouched rows, identical bits
@pytest.mark.parametrize("row0", [0, 37])
def test_gradients_are_added_and_other_rows_left_alone(ops, row0):
    d, B, N, q, tau = 48, 129, 127, 5, 0.2
    Fp, Ep, AS, P, idv = _case("accumulate", d, B, N, q, row0)
    gen = _gen("pattern")
    base = (torch.randn(Fp.shape, generator=gen), torch.randn(Ep.shape, generator=gen))
    loss0, gF0, gE0, dP0 = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau)
    loss1, gF1, gE1, dP1 = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau, base=base)
    assert torch.equal(loss0, loss1) and torch.equal(dP0, dP1)  # dP is stored, not added
    table = torch.zeros(Fp.shape[0], dtype=torch.bool)
    table[row0:row0 + N] = True
    batch = torch.zeros(Fp.shape[0], dtype=torch.bool)
    batch[row0 + idv] = True
    assert torch.equal(gF1[~table], base[0][~table]) and torch.equal(gE1[~batch], base[1][~batch])  # bit-unchanged
    assert float(gF0[~table].abs().max()) == 0 and float(gE0[~batch].abs().max()) == 0
    # pattern + gradient.  A row receives one addition for the dense part (g_final) and one per occurrence of its id, each
    # rounded to half a unit in the last place of the running total; the run from zero carries the same roundings on the
    # gradient alone
    most = int(torch.bincount(idv).max())
    for got, g0, b0, rows, adds in ((gF1, gF0, base[0], table, 1 + most), (gE1, gE0, base[1], batch, most)):
        want = b0[rows].double() + g0[rows].double()
        tol = adds * (ULP / 2) * (float(want.abs().max()) + float(g0[rows].abs().max()))
        assert float((got[rows].double() - want).abs().max()) <= tol
        assert not torch.equal(got[rows], b0[rows])


def test_two_runs_and_the_loss_only_call_give_the_same_bits(ops):
    d, B, N, q, row0, tau = 64, 300, 1000, 5, 37, 0.2
    Fp, Ep, AS, P, idv = _case("bits", d, B, N, q, row0)
    a = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau, upstream=(0.5, -0.5))
    b = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau, upstream=(0.5, -0.5))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau, grads=False)
    assert torch.equal(a[0], c[0])


# ========================================================================================= (e) the projection and the expansion
LR_GRID = [(1, 1, 32), (255, 5, 48), (4097, 16, 256), (4097, 5, 32), (255, 16, 256), (1, 16, 48), (4097, 1, 48)]


def _lr_tol(yard, want):
    return max(2 * _rel(yard, want), ULP)


@pytest.mark.parametrize("n,q,d", LR_GRID)
def test_lowrank_project_and_expand_vs_float64(ops, n, q, d):
    gen = _gen("lowrank", n, q, d)
    A_wide, X_wide = torch.randn(n, q + 3, generator=gen), torch.randn(n, d + 8, generator=gen)
    A, X = A_wide[:, 1:1 + q], X_wide[:, 4:4 + d]  # row strides wider than the rows
    assert n == 1 or not A.is_contiguous()
    Ad, Xd = A_wide.cuda()[:, 1:1 + q], X_wide.cuda()[:, 4:4 + d]
    want = A.double().t() @ X.double()
    got = ops.lowrank_project_raw(Ad, Xd).cpu()
    e, tol = _rel(got, want), _lr_tol(A.t() @ X, want)
    print("  project n=%d q=%d d=%d: %.3e of the largest entry (bound %.3e)" % (n, q, d, e, tol))
    assert got.shape == (q, d) and e <= tol
    assert torch.equal(got, ops.lowrank_project_raw(Ad, Xd).cpu())  # the same bits on a second run
    # accumulate: out += A^T X
    out = torch.ones(q, d, device="cuda")
    ops.lowrank_project_raw(Ad, Xd, out=out, accumulate=True)
    assert _rel(out.cpu(), want + 1) <= tol + ULP
    # the row-id form with repeats: sum_r A[rows[r]]^T X[r]
    rows = torch.randint(0, n, (n,), generator=gen)
    if n >= 2:
        rows[1] = rows[0]
    want_r = A[rows].double().t() @ X.double()
    got_r = ops.lowrank_project_raw(Ad, Xd, a_rows=rows.cuda()).cpu()
    assert _rel(got_r, want_r) <= _lr_tol(A[rows].t() @ X, want_r)
    # the expansion into a wider panel, stored then accumulated with a scale
    P = torch.randn(q, d, generator=gen)
    Y_wide = torch.full((n, d + 8), 7.0, device="cuda")
    Y = Y_wide[:, 4:4 + d]
    ops.lowrank_expand_raw(Ad, P.cuda(), Y=Y)
    want_y = A.double() @ P.double()
    tol_y = _lr_tol(A @ P, want_y)
    assert _rel(Y.cpu(), want_y) <= tol_y
    ops.lowrank_expand_raw(Ad, P.cuda(), Y=Y, scale=-0.5, accumulate=True)
    assert _rel(Y.cpu(), 0.5 * want_y) <= tol_y + ULP
    keep = torch.ones(d + 8, dtype=torch.bool)
    keep[4:4 + d] = False
    assert float((Y_wide.cpu()[:, keep] - 7.0).abs().max()) == 0  # the columns beside the rows are untouched
    got_e = ops.lowrank_expand_raw(Ad, P.cuda(), a_rows=rows.cuda(), scale=2.0).cpu()
    assert got_e.shape == (n, d) and _rel(got_e, 2 * (A[rows].double() @ P.double())) <= _lr_tol(2 * (A[rows] @ P), 2 * (A[rows].double() @ P.double()))


def test_lowrank_operators_under_autograd(ops):
    n, q, d = 255, 5, 48
    gen = _gen("lowrank-autograd")
    A, X, P = torch.randn(n, q, generator=gen), torch.randn(n, d, generator=gen), torch.randn(q, d, generator=gen)
    W1, W2 = torch.randn(q, d, generator=gen), torch.randn(n, d, generator=gen)
    Xd, Pd = X.cuda().requires_grad_(True), P.cuda().requires_grad_(True)
    (ops.lowrank_project(A.cuda(), Xd) * W1.cuda()).sum().backward()
    (ops.lowrank_expand(A.cuda(), Pd, scale=0.5) * W2.cuda()).sum().backward()
    want_x, want_p = A.double() @ W1.double(), 0.5 * (A.double().t() @ W2.double())
    assert _rel(Xd.grad.cpu(), want_x) <= _lr_tol(A @ W1, want_x) and _rel(Pd.grad.cpu(), want_p) <= _lr_tol(0.5 * (A.t() @ W2), want_p)


# ================================================================================================================ (f) autograd
def test_autograd_is_the_raw_call(ops):
    d, B, N, q, row0, tau = 48, 127, 129, 5, 37, 0.2
    Fp, Ep, AS, P, idv = _case("autograd", d, B, N, q, row0)
    Fd, Ed, Pd = (t.cuda().requires_grad_(True) for t in (Fp, Ep, P))
    lse, pos = ops.svd_nce_loss(Fd, Ed, row0, N, AS.cuda(), Pd, idv.cuda(), tau)
    (0.7 * lse - 1.3 * pos).backward()
    loss, gF, gE, dP = _run(ops, Fp, Ep, row0, N, AS, P, idv, tau, upstream=(0.7, -1.3))
    assert float(lse) == float(loss[0]) and float(pos) == float(loss[1])
    assert torch.equal(Fd.grad.cpu(), gF) and torch.equal(Ed.grad.cpu(), gE) and torch.equal(Pd.grad.cpu(), dP)


# ============================================================================================================ (g) (h) engine, plugin
@pytest.fixture(scope="module")
def golden_lightgcl():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "lightgcl_small.npz"), allow_pickle=False))


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCL.txt"), "LightGCL")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _statement_inputs(g, tag, gs):
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.symmetric_operator(g["R_indptr"], g["R_indices"], g["R_data"], U, n - U)
    E0 = torch.from_numpy(np.concatenate([g["%s_init_%s" % (tag, p)] for p in PARAMS])).double()
    f = [torch.from_numpy(g[tag + k]).double() for k in ("_svd_u", "_s", "_svd_v")]
    reg, ssl, tau, K, q, lr = g[tag + "_hyper"].tolist()
    return A, E0, f, dict(reg=reg, ssl=ssl, tau=tau, K=int(K), q=int(q), lr=lr), U


def _model(tmp_path, golden_small, g, tag, **over):
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools
    from models.LightGCL import LightGCL

    reg, ssl, tau, K, q, lr = g[tag + "_hyper"].tolist()
    cfg = _cfg(GCN_layer=int(K), svd_q=int(q), temperature=tau, ssl_lambda=ssl, reg_lambda=reg, learn_rate=lr, embedding_size=32)
    cfg.update({k: str(v) for k, v in over.items()})
    d = tmp_path / "small"
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(golden_small["train_txt"].tobytes())
    (d / "test.txt").write_bytes(golden_small["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(d), cfg)
    tools.set_seed(2024)

    class Fed(LightGCL):  # the reference's recorded factors in place of this process's torch.svd_lowrank draw
        factor_source = tuple(g[tag + k] for k in ("_svd_u", "_s", "_svd_v"))

    m = Fed(cfg, data, torch.device("cuda")).to("cuda")
    prm = {p: getattr(m, p).weight for p in PARAMS}
    if int(cfg["embedding_size"]) == 32:  # the fixture's tables (another width keeps its own xavier draw)
        with torch.no_grad():
            for p in PARAMS:
                prm[p].copy_(torch.from_numpy(g["%s_init_%s" % (tag, p)]))
    return cfg, m, prm


def _tables_check(what, mine, want):
    off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
    print("  %-60s outside rtol 1e-4 / atol 1e-6: %.3g of the elements, largest difference %.3g" % (what, off.mean(), np.abs(mine - want).max()))
    assert off.mean() < 1e-3 and np.abs(mine - want).max() < 1e-4, (what, off.mean(), np.abs(mine - want).max())


@pytest.mark.parametrize("tag", ["def", "clamp"])
def test_fused_steps_match_the_fixtures_trajectory(ops, tag, tmp_path, golden_small, golden_lightgcl):
    g = golden_lightgcl
    A, E0, (su, s, sv), h, U = _statement_inputs(g, tag, golden_small)
    tri = torch.from_numpy(g["traj_batches"])
    batches = [tri[i * 128:(i + 1) * 128] for i in range(3)]
    _, panels = ref.adam_steps(A, E0, su, s, sv, batches, h["K"], h["reg"], h["ssl"], h["tau"], U, h["lr"])
    cfg, m, prm = _model(tmp_path, golden_small, g, tag)
    assert m.fused_step_available() and m.n_layers == h["K"] and m.svd_q == h["q"]
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 3), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 128:(i + 1) * 128, c].contiguous().cuda() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
        mine = np.concatenate([prm[p].detach().cpu().numpy() for p in PARAMS])
        _tables_check("%s tables after step %d vs float64" % (tag, i + 1), mine, panels[i].numpy())
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=LOSS_RTOL, atol=1e-9)
    for p in PARAMS:
        _tables_check("%s trajectory %s vs the fixture" % (tag, p), prm[p].detach().cpu().numpy(), g["%s_traj_%s" % (tag, p)])
    assert all(int(opt.state[q_]["step"]) == 3 for q_ in m.parameters())


@pytest.mark.parametrize("tag,layers", [("def", None), ("clamp", None), ("def", 1)])
def test_fused_step_matches_float64_and_forward_plus_autograd(ops, tag, layers, tmp_path, golden_small, golden_lightgcl):
    g = golden_lightgcl
    A, E0, (su, s, sv), h, U = _statement_inputs(g, tag, golden_small)
    K = h["K"] if layers is None else layers
    bb = torch.from_numpy(g["batch"])
    want_l, want_g, want_F, _ = ref.step64(A, E0, su, s, sv, bb[:, 0], bb[:, 1], bb[:, 2], K, h["reg"], h["ssl"], h["tau"], U)
    if layers is None:
        np.testing.assert_allclose(want_l.numpy(), g[tag + "_loss"], rtol=1e-10)  # the statement is the fixture's
    l32, g32, _, _ = ref.step64(A, E0, su, s, sv, bb[:, 0], bb[:, 1], bb[:, 2], K, h["reg"], h["ssl"], h["tau"], U, dtype=F32,
                                layered=True)
    tol = max(2 * _rel(g32, want_g), ULP)
    b = tuple(bb[:, c].contiguous().cuda() for c in range(3))
    over = {} if layers is None else dict(GCN_layer=layers)
    # forward() + autograd + the same Adam kernel
    cfg, m, prm = _model(tmp_path, golden_small, g, tag, **over)
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    ll = m(*b)
    assert len(ll) == 3
    opt.zero_grad()
    sum(ll).backward()
    grad_a = torch.cat([prm[p].grad.cpu() for p in PARAMS])
    opt.step()
    loss_a = np.array([x.item() for x in ll])
    tables_a = np.concatenate([prm[p].detach().cpu().numpy() for p in PARAMS])
    # the fused step from the same tables
    cfg, m2, prm2 = _model(tmp_path, golden_small, g, tag, **over)
    opt2 = ops.Adam(m2.parameters(), lr=float(cfg["learn_rate"]))
    eng = m2.lightgcl_engine()
    assert eng.K == K
    loss_f = torch.zeros(3, device="cuda")
    assert m2.fused_train_step(*b, loss_f, opt2)
    grad_f = eng.GRAD.cpu()
    e_a, e_f = _rel(grad_a, want_g), _rel(grad_f, want_g)
    print("  %s K=%d: gradient of forward() + autograd %.3e, of the fused step %.3e of the largest entry from float64 "
          "(float32 torch %.3e, bound %.3e); fused vs autograd %.3e" % (tag, K, e_a, e_f, _rel(g32, want_g), tol, _rel(grad_f, grad_a)))
    np.testing.assert_allclose(loss_a, want_l.numpy(), rtol=LOSS_RTOL, atol=1e-9)
    np.testing.assert_allclose(loss_f.cpu().numpy(), want_l.numpy(), rtol=LOSS_RTOL, atol=1e-9)
    assert e_a <= tol and e_f <= tol
    tables_f = np.concatenate([prm2[p].detach().cpu().numpy() for p in PARAMS])
    _tables_check("%s K=%d tables after Adam, fused vs forward() + autograd" % (tag, K), tables_f, tables_a)
    assert not np.array_equal(tables_f, E0.float().numpy())
    # the rating, against the float64 rows the step started from
    m.eval()
    cfg, m3, _ = _model(tmp_path, golden_small, g, tag, **over)
    m3.eval()
    users = torch.from_numpy(g["rating_users"]).cuda()
    rating = torch.sigmoid(want_F[g["rating_users"]] @ want_F[U:].t()).numpy()
    np.testing.assert_allclose(m3.get_rating_for_test(users).cpu().numpy(), rating, rtol=1e-4, atol=1e-5)
    if layers is None:
        np.testing.assert_allclose(rating, g[tag + "_rating"], rtol=1e-6, atol=1e-7)


def test_engine_refuses_what_it_cannot_run(ops, tmp_path, golden_small, golden_lightgcl):
    from idgrec_amd.lightgcl import LightgclEngine

    g = golden_lightgcl
    cfg, m, prm = _model(tmp_path, golden_small, g, "def")
    f = [torch.from_numpy(g["def" + k]).cuda() for k in ("_svd_u", "_s", "_svd_v")]
    with pytest.raises(ValueError, match="GCN_layer >= 1"):
        LightgclEngine(m.Graph, 300, 250, m._storage, 0, *f)
    with pytest.raises(ValueError, match="factors"):
        LightgclEngine(m.Graph, 300, 250, m._storage, 2, f[0][:10], f[1], f[2])
    with pytest.raises(ValueError, match="d = 48"):
        LightgclEngine(m.Graph, 300, 250, torch.zeros(550, 48, device="cuda"), 2, *f)
    cfg, m48, _ = _model(tmp_path, golden_small, g, "def", embedding_size=48)
    assert not m48.fused_step_available()  # trains through the differentiable operators
    b = tuple(torch.from_numpy(g["batch"][:, c].copy()).cuda() for c in range(3))
    ll = m48(*b)
    sum(ll).backward()
    assert all(np.isfinite(x.item()) for x in ll) and float(m48.user_embedding.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("width,fused", [(64, True), (48, False)])
def test_trainer_end_to_end(width, fused, tmp_path):
    """One epoch through the plugin surface as scripts/e2e_epoch.py drives it: generated dataset files -> Data -> Trainer.train(),
    with this process's own torch.svd_lowrank factors."""
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    S.make_dataset(str(tmp_path), "tiny", n_test=2)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", training_epochs=1, interval=1, batch_size=64, test_batch_size=64,
               top_K="[5, 10]", embedding_size=width, learn_rate=0.01)
    stream = io.StringIO()
    logger = logging.getLogger("lightgcl_e2e_%d" % width)
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    data = data_loader.Data(cfg["dataset_path"] + cfg["dataset"], cfg)
    tr = importlib.import_module("models.LightGCL").Trainer(None, cfg, data, torch.device("cuda"), logger)
    m = tr.model
    assert m.svd_u.shape == (data.num_users, 5) and m.svd_v.shape == (data.num_items, 5) and m.svd_u.is_cuda
    w0 = m.user_embedding.weight.detach().cpu().clone()
    tr.train()
    assert m.fused_step_available() == fused
    lines = stream.getvalue().splitlines()
    loss_lines = [ln for ln in lines if "training loss" in ln]
    assert len(loss_lines) == 1 and "Model training process completed." in lines
    nums = [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", loss_lines[0].split("training loss:")[1])]
    assert len(nums) == 4 and np.isfinite(nums).all() and abs(nums[0] - sum(nums[1:])) < 1e-4
    assert any("Test recall" in ln for ln in lines)
    assert not torch.equal(m.user_embedding.weight.detach().cpu(), w0)
