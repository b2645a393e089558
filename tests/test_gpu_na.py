"""LightCCF / LightCSCF on the GPU: idg_na_nce_f32 against the float64 statement (tests/na_ref64.py) across its tile edges,
widths, temperatures and both forms of f; the same bits with and without gradients, with a plan built ahead, in a fresh
workspace and run to run; ops.na_nce_loss under autograd; ops.reg_rows_raw against float64; models.LightCCF and
models.LightCSCF against the reference's fixture (both encoders each), their fused steps against the reference's Adam
trajectory and against forward() + autograd; training end to end.

Tolerances.  Losses rtol 1e-5, tables after Adam rtol 1e-4 / atol 1e-6 (the siblings' bounds); the trajectory by
tests/test_gpu_bigcf.py's criterion (under 1e-3 of a table's elements outside that band, none further than 1e-4 — which the
reference's own float32 run meets: tests/test_na_host.py).
Gradients: GRAD_TOL = 1e-5 of the largest entry of the float64 gradient.  Derivation: the bound is twice the worst float32
yardstick tests/test_na_host.py measures (the reference's expressions in float32 against the float64 statement, over this
file's grid, its extra case, its riders and the fixture), capped by the siblings' 1e-5.  That yardstick is 3.2e-2 — LightCCF
at T = 0.05, B = 129, d = 64, where nearly all of every row sum sits on the diagonal and on the columns that repeat the row's
user, so that the gradient is the 1e5 times smaller rest of parts that cancel, and a float32 evaluation of those parts is
wrong by percents of it; next come one user repeated 96 times at T = 0.1 (1.8e-5) and the LightCCF cases of the grid at T = 0.1
(up to 4.5e-6).  Twice 3.2e-2 is far above the cap, so the cap IS the bound: 1e-5, for every case, T = 0.05 included.  (It is
what made the kernel a double-precision one: csrc/idg_nance.hip)
The cases over the widths of tests/widths.py (EVERY_NDT at B = 129 and 257, T = 0.1, both forms of f; the regulariser at
B = 129), which with the grid launch every NDT = ceil(d / 32) = 1 .. 8 the source instantiates, take the same GRAD_TOL: their
float32 yardsticks are 9.7e-7 .. 4.3e-6 (worst: LightCCF, B = 257, d = 224; tests/test_na_host.py prints each), twice which
is under the cap in every case — and the double-precision kernel sits far below either.
At B = 1 the gradient is zero (LightCCF) or a rest of the same kind; the error is then divided by the scale of the parts
(na_ref64.grad_scale has the reasoning).  A zero panel row's own gradient carries normalize()'s 1e12 and is compared on its
own scale, at 1e-4.  Every LightCSCF case asserts, in float64, that no score lies within 1e-5 of the margin.

Measured on an MI355X (131 tests, 32 s).  The kernel's gradients over the grid: at most 1.8e-7 of the largest entry = 0.018 of
GRAD_TOL at T = 0.1 (B = 127, d = 64, LightCCF), 7.7e-8 at T = 1, 3.2e-8 at B = 1 (on the parts' scale); the extra case at
T = 0.05: 5.2e-7 = 0.052 of GRAD_TOL (LightCCF, the case whose float32 yardstick is 3.2e-2) and 2.4e-7 (LightCSCF); the riders:
all-distinct ids 8.3e-8, one repeated user 2.3e-7 (B = 96, LightCCF: yardstick 1.8e-5), zero rows 7.1e-8 (the zero rows
themselves 5.1e-8 on their own scale), store / accumulate 1.6e-7.  What is left is the one rounding of the double result to the
float32 panel and the float32 form in which temperature and margin reach the library.  Losses within 5.9e-8 relative.
ops.reg_rows_raw: loss within 5.5e-8, gradient within 6.0e-8 (bound 2^-23).  The plugins' .grad against the fixture: 6.7e-8
(`ccf_mf`), 1.6e-7 (`ccf_gcn`), 9.5e-8 (`cscf_mf`), 2.2e-7 (`cscf_gcn`); three fused steps: no element outside rtol 1e-4 /
atol 1e-6 in any setting, 3.2e-6 off at most (`ccf_gcn`); the fused step's gradient equals forward() + autograd's bit for bit
(the same kernels in the same order); the float-atomic path of the engine within 6.0e-8 of the deterministic one.
With the cases over every built width (181 tests, 4.4 s; the 50 new cases under 0.1 s together): gradients at most 1.6e-7 of
the largest entry = 0.016 of GRAD_TOL (B = 257, d = 192, LightCCF), losses within 4.9e-8 relative; ops.reg_rows_raw at B = 129
over the same widths: loss within 3.5e-8, gradient within 5.1e-8 (bound 2^-23).
"""
import importlib
import io
import logging
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import na_ref64 as ref  # noqa: E402
from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 1e-5
TAGS = tuple(ref.SETTINGS)


@pytest.fixture(scope="module")
def golden_na():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "na_small.npz")))


def _cfg(name, **kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", name + ".txt"), name)
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _small_data(tmp_path, g, cfg):
    import utility.utility_data.data_loader as data_loader

    d = tmp_path / "small"
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    return data_loader.Data(str(d), cfg)


def _check(loss, g, panel, U, users, pos, t, margin, weight=1.0, upstream=None, skip_rows=None, what=""):
    """The loss at rtol 1e-5 and the gradient at GRAD_TOL against the float64 literal form; prints every figure first."""
    if margin is not None:
        gap = ref.kink_distance(panel, U, users, pos, margin)
        assert gap > ref.KINK_GAP, (what, gap)
    l64, g64 = ref.panel_terms(panel.cpu(), U, users.cpu(), pos.cpu(), t, margin, weight, upstream=upstream)
    e_l = abs(float(loss.double().cpu()) - float(l64)) / abs(float(l64))
    keep = torch.ones(panel.shape[0], dtype=torch.bool)
    if skip_rows:
        keep[list(skip_rows)] = False
    scale = ref.grad_scale(panel, U, users, pos, t, margin, g64[keep], weight, upstream)
    e_g = float((g.double().cpu() - g64)[keep].abs().max()) / scale
    print("%s: loss %.2e (relative), gradient %.2e of the largest entry = %.2g of GRAD_TOL" % (what, e_l, e_g, e_g / GRAD_TOL))
    assert e_l <= 1e-5, (what, e_l)
    assert e_g <= GRAD_TOL, (what, e_g)
    for r in skip_rows or ():
        e_r = float((g[r].double().cpu() - g64[r]).abs().max() / g64[r].abs().max())
        print("%s: zero row %d on its own scale %.2e" % (what, r, e_r))
        assert e_r <= 1e-4, (what, r, e_r)
    return l64, g64


def _up(x):
    return None if x is None else torch.tensor([x], dtype=torch.float32, device="cuda")


# --------------------------------------------------------------------------------------- (a) the grid
@pytest.mark.parametrize("margin", ref.GRID_M)
@pytest.mark.parametrize("t", ref.GRID_T)
@pytest.mark.parametrize("d", ref.GRID_D)
@pytest.mark.parametrize("B", ref.GRID_B)
def test_op_matches_float64_statement(B, d, t, margin):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, ref.grid_seed(B, d, t), device="cuda")
    up = ref.grid_upstream(B)
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, g, upstream=_up(up))
    _check(loss, g, panel, U, users, pos, t, margin, upstream=up, what="B=%d d=%d T=%g margin=%s" % (B, d, t, margin))
    if B >= 96:
        assert int(torch.unique(users).numel()) < B and int(torch.unique(pos).numel()) < B  # 45 / 61 rows: ids repeat


@pytest.mark.parametrize("margin", ref.GRID_M)
@pytest.mark.parametrize("d", widths.EVERY_NDT)
@pytest.mark.parametrize("B", ref.WIDTH_B)
def test_op_matches_float64_statement_over_every_built_width(B, d, margin):
    """Every NDT = ceil(d / 32) the source instantiates, both forms of f, with gradients and, at B = 129, through the loss-only
    call too (the same bits)."""
    from idgrec_amd import ops

    t = ref.WIDTH_T
    panel, users, pos, U = ref.case_inputs(B, d, ref.width_seed(B, d), device="cuda")
    up = ref.grid_upstream(B)
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, g, upstream=_up(up)).clone()
    _check(loss, g, panel, U, users, pos, t, margin, upstream=up,
           what="widths B=%d d=%d (NDT %d) T=%g margin=%s" % (B, d, widths.ndt(d), t, margin))
    if B == 129:
        l0 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0).clone()
        assert torch.equal(l0, loss)  # the loss alone: the same bits as with gradients


@pytest.mark.parametrize("margin", ref.GRID_M)
def test_op_at_the_low_end_of_the_temperature_range(margin):
    from idgrec_amd import ops

    B, d, t = ref.EXTRA
    panel, users, pos, U = ref.case_inputs(B, d, ref.grid_seed(B, d, t), device="cuda")
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 5.0, g)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
    _check(loss, g, panel, U, users, pos, t, margin, weight=5.0, what="B=%d d=%d T=%g margin=%s" % (B, d, t, margin))


def _riders(*forms):
    return [c for c in ref.RIDERS if c[0] in forms]


@pytest.mark.parametrize("form,B,d,t,margin,seed", _riders("distinct", "one_user"))
def test_op_on_distinct_ids_and_one_repeated_user(form, B, d, t, margin, seed):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, seed, device="cuda", form=form)
    assert int(torch.unique(users).numel()) == (B if form == "distinct" else 1)
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, g)
    _check(loss, g, panel, U, users, pos, t, margin, what="%s B=%d d=%d T=%g margin=%s" % (form, B, d, t, margin))


@pytest.mark.parametrize("form,B,d,t,margin,seed", _riders("zero_rows"))
def test_op_with_a_zero_row_as_user_and_as_positive(form, B, d, t, margin, seed):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, seed, device="cuda", form=form)
    zu, zp = ref.zero_rows_of(users, pos, U)
    assert float(panel[zu].abs().max()) == 0 and float(panel[zp].abs().max()) == 0
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, g)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
    _check(loss, g, panel, U, users, pos, t, margin, skip_rows=(zu, zp), what="zero rows B=%d d=%d T=%g margin=%s" % (B, d, t, margin))


@pytest.mark.parametrize("form,B,d,t,margin,seed", _riders("random"))
def test_op_accumulates_and_stores(form, B, d, t, margin, seed):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, seed, device="cuda")
    n = panel.shape[0]
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, g)
    rows = torch.zeros(n, dtype=torch.bool, device="cuda")
    rows[users] = True
    rows[U + pos] = True
    if B == 127:  # leave rows outside the batch
        assert not bool(rows.all())
    # accumulate = 1 into a pre-filled panel: added
    gen = torch.Generator(device="cuda").manual_seed(B)
    fill = torch.randn(panel.shape, device="cuda", generator=gen) * float(g.abs().max())
    acc = fill.clone()
    ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, acc)
    assert torch.equal(acc[rows], (fill + g)[rows]) and torch.equal(acc[~rows], fill[~rows])
    # accumulate = 0 into a sentinel: the batch's rows hold the gradient, every other element keeps its bits
    sent = float.fromhex("0x1.234566p+3")
    st = torch.full_like(panel, sent)
    loss2 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, st, accumulate=False)
    assert torch.equal(st[rows], g[rows]) and bool((st[~rows] == sent).all())
    assert torch.equal(loss2, loss)
    # ... and with the plan of a batch WITH negatives (the engine's): their rows are stored too, as zeros where no user or
    # positive of the batch shares them
    neg = torch.randint(0, n - U, (B,), generator=torch.Generator().manual_seed(B + 1)).cuda()
    plan = ops.bpr_workspace(B, d, "cuda")
    ops.bpr_plan_raw(users, pos, neg, U, n, d, ws=plan)
    st3 = torch.full_like(panel, sent)
    ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, st3, accumulate=False, plan_ws=plan)
    only_neg = torch.zeros(n, dtype=torch.bool, device="cuda")
    only_neg[U + neg] = True
    only_neg &= ~rows
    assert torch.equal(st3[rows], g[rows]) and bool((st3[only_neg] == 0).all()) and bool((st3[~(rows | only_neg)] == sent).all())
    acc3 = fill.clone()
    ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 1.0, acc3, plan_ws=plan)
    assert torch.equal(acc3, acc)
    _check(loss, g, panel, U, users, pos, t, margin, what="store / accumulate B=%d d=%d T=%g margin=%s" % (B, d, t, margin))


# --------------------------------------------------------------------------------------- (b) the same bits
@pytest.mark.parametrize("B,d,t,margin", [(1, 64, 0.1, None), (129, 100, 0.1, 0.7), (257, 256, 1.0, None)])
def test_same_bits_loss_only_planned_and_rerun(B, d, t, margin):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, 7 * B + d, device="cuda")
    g1, g2, g3 = (torch.zeros_like(panel) for _ in range(3))
    l1 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 2.0, g1).clone()
    l0 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 2.0).clone()
    assert torch.equal(l0, l1)  # the loss alone: the same bits as with gradients
    l2 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 2.0, g2, ws=ops.na_nce_workspace(B, d, "cuda")).clone()
    assert torch.equal(l2, l1) and torch.equal(g2, g1)  # run to run (and in a fresh workspace)
    plan = ops.bpr_workspace(B, d, "cuda")
    ops.bpr_plan_raw(users, pos, pos, U, panel.shape[0], d, ws=plan)
    l3 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 2.0, g3, plan_ws=plan).clone()
    l4 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 2.0, plan_ws=plan).clone()
    assert torch.equal(l3, l1) and torch.equal(g3, g1) and torch.equal(l4, l1)
    g5 = torch.zeros_like(panel)
    l5 = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 2.0, g5).clone()
    assert torch.equal(l5, l1) and torch.equal(g5, g1)  # a rerun in the cached workspace


# --------------------------------------------------------------------------------------- (c) operators
@pytest.mark.parametrize("d,margin", [(48, None), (64, 0.7)])
def test_op_under_autograd_equals_the_raw_call(d, margin):
    from idgrec_amd import ops

    B, t = 129, 0.2
    panel, users, pos, U = ref.case_inputs(B, d, 5 * d, device="cuda")
    p = panel.clone().requires_grad_(True)
    na = ops.na_nce_loss(p, users, pos, U, t, margin, 5.0)
    (-1.3 * na).backward()
    g = torch.zeros_like(panel)
    loss = ops.na_nce_loss_raw(panel, users, pos, U, t, margin, 5.0, g, upstream=_up(-1.3))
    assert torch.equal(na.detach().reshape(1), loss) and torch.equal(p.grad, g)
    _check(loss, g, panel, U, users, pos, t, margin, weight=5.0, upstream=-1.3, what="autograd d=%d margin=%s" % (d, margin))


@pytest.mark.parametrize("B,d", [(1, 64), (96, 48), (129, 100), (257, 256)])
def test_reg_rows_against_float64(B, d):
    """The regulariser alone: duplicate negatives, negatives equal to positives, rows outside the batch untouched."""
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, 3 * B + d, device="cuda")
    n, lam = panel.shape[0], 0.05
    neg = torch.randint(0, n - U, (B,), generator=torch.Generator().manual_seed(B)).cuda()
    neg[::3] = pos[::3]  # negatives equal to positives
    if B > 4:
        neg[1] = neg[4]  # a repeated negative
    l64, g64 = ref.reg64(panel.cpu(), U, users.cpu(), pos.cpu(), neg.cpu(), lam)
    sent = float.fromhex("0x1.234566p+3")
    ge, gf = torch.full_like(panel, sent), torch.full_like(panel, sent)
    loss = ops.reg_rows_raw(panel, users, pos, neg, U, lam, g_ego=ge, g_final=gf)
    rows = torch.zeros(n, dtype=torch.bool, device="cuda")
    rows[users] = True
    rows[U + pos] = True
    rows[U + neg] = True
    e_l = abs(float(loss) - float(l64)) / float(l64)
    e_g = float((ge[rows].double().cpu() - g64[rows.cpu()]).abs().max() / g64.abs().max())
    print("reg rows B=%d d=%d: loss %.2e (relative), gradient %.2e of the largest entry" % (B, d, e_l, e_g))
    # two float32 roundings, 2^-24 each: reg_lambda reaches the library as a float32, and the float64 sum is rounded once
    # (the loss adds nothing visible: its sums are in double)
    assert e_l <= 2.0 ** -23 and e_g <= 2.0 ** -23
    assert bool((gf[rows] == 0).all()) and bool((gf[~rows] == sent).all()) and bool((ge[~rows] == sent).all())
    # a plan built ahead, the loss alone: the same bits
    plan = ops.bpr_workspace(B, d, "cuda")
    ops.bpr_plan_raw(users, pos, neg, U, n, d, ws=plan)
    ge2 = torch.full_like(panel, sent)
    l2 = ops.reg_rows_raw(panel, users, pos, neg, U, lam, g_ego=ge2, plan_ws=plan)
    l3 = ops.reg_rows_raw(panel, users, pos, neg, U, lam)
    assert torch.equal(l2, loss) and torch.equal(l3, loss) and torch.equal(ge2, ge)
    # under autograd
    p = panel.clone().requires_grad_(True)
    (2.0 * ops.reg_rows_loss(p, users, pos, neg, U, lam)).backward()
    assert torch.equal(p.grad[rows], 2.0 * ge[rows]) and bool((p.grad[~rows] == 0).all())


@pytest.mark.parametrize("d", widths.EVERY_NDT)
def test_reg_rows_against_float64_over_every_built_width(d):
    test_reg_rows_against_float64(129, d)


# --------------------------------------------------------------------------------------- (d) the models
def _model(tag, g, tmp_path, golden_small, **kw):
    import utility.utility_function.tools as tools

    name, enc = ref.SETTINGS[tag]
    t, layers, lr, reg, weight, margin, d = g[tag + "_hyper"].tolist()
    own = dict(reg_lambda=reg, ssl_lambda=weight) if name == "LightCCF" else dict(lambda_reg=reg, lambda_gamma=weight, lambda_margin=margin)
    own.update(encoder=enc, temperature=t, GCN_layer=int(layers), learn_rate=lr, embedding_size=int(d))
    own.update(kw)
    cfg = _cfg(name, **own)
    data = _small_data(tmp_path, golden_small, cfg)
    tools.set_seed(2024)
    cls = getattr(importlib.import_module("models." + name), name)
    return cls(cfg, data, torch.device("cuda")).to("cuda"), cfg, data


def _n_losses(tag):
    return 2 if tag == "cscf_gcn" else 3


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_fixture(tag, tmp_path, golden_small, golden_na):
    from idgrec_amd import ops

    g = golden_na
    d = int(g[tag + "_hyper"][6])
    m, cfg, data = _model(tag, g, tmp_path, golden_small)
    assert m.n_fused_losses == _n_losses(tag)
    np.testing.assert_array_equal(m.user_embedding.weight.detach().cpu().numpy(), g["init%d_user_embedding" % d])
    b = torch.from_numpy(g["batch"]).cuda()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == _n_losses(tag)
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-5)
    sum(ll).backward()
    for p in ("user_embedding", "item_embedding"):
        want = g["%s_grad_%s" % (tag, p)]
        e = float(np.abs(getattr(m, p).weight.grad.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print("%s %s.grad: %.2e of the largest entry = %.2g of GRAD_TOL" % (tag, p, e, e / GRAD_TOL))
        assert e <= GRAD_TOL, (p, e)
    m.eval()
    rating = m.get_rating_for_test(torch.from_numpy(g["rating_users"]).cuda())
    np.testing.assert_allclose(rating.cpu().numpy(), g[tag + "_rating"], rtol=1e-5, atol=1e-6)
    # three fused steps against the reference's own Adam trajectory
    m, cfg, data = _model(tag, g, tmp_path, golden_small)
    assert m.fused_step_available()
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, _n_losses(tag)), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        assert m.fused_train_step(*bt, loss[i], opt)
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    for p in ("user_embedding", "item_embedding"):
        mine, want = getattr(m, p).weight.detach().cpu().numpy(), g["%s_traj_%s" % (tag, p)]
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("%s %s after three steps: %.2e of the elements outside the band, at most %.2e off" % (tag, p, off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, (p, off.mean())
        assert np.abs(mine - want).max() < 1e-4, (p, np.abs(mine - want).max())


@pytest.mark.parametrize("tag", TAGS)
def test_fused_step_equals_autograd_step(tag, tmp_path, golden_small, golden_na):
    from idgrec_amd import ops

    g = golden_na
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    bt = tuple(tri[:256, c].contiguous() for c in range(3))
    res = []
    for fused in (True, False):
        m, cfg, data = _model(tag, g, tmp_path, golden_small)
        m.keep_fused_grad = True
        opt = ops.Adam(m.parameters(), lr=0.001)
        loss = torch.zeros(_n_losses(tag), device="cuda")
        if fused:
            assert m.fused_train_step(*bt, loss, opt)
        else:
            ll = m(*bt)
            loss = torch.stack([x.detach() for x in ll])
            opt.zero_grad()
            sum(ll).backward()
            opt.step()
        res.append((loss.cpu().numpy(), torch.cat([m.user_embedding.weight.grad, m.item_embedding.weight.grad]).cpu().numpy(),
                    m._storage.detach().cpu().numpy()))
    (l_f, g_f, w_f), (l_a, g_a, w_a) = res
    np.testing.assert_allclose(l_f, l_a, rtol=1e-5)
    e = float(np.abs(g_f.astype(np.float64) - g_a).max() / np.abs(g_a).max())
    print("%s fused against autograd: gradient %.2e of the largest entry" % (tag, e))
    assert e <= GRAD_TOL
    np.testing.assert_allclose(w_f, w_a, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("other", ["au", "sccf"])
def test_engine_refuses_na_with_au_or_sccf(other, tmp_path, golden_small, golden_na):
    m, cfg, data = _model("cscf_mf", golden_na, tmp_path, golden_small)
    eng = m.engine()
    assert eng.na == (m.temperature, m.lambda_gamma, m.margin, True) and eng.au is None and eng.sccf is None
    setattr(eng, other, (2.0,) if other == "au" else (0.1,))
    b = torch.from_numpy(golden_na["batch"]).cuda()
    with pytest.raises(ValueError, match="na joins"):
        eng.loss_and_grad(b[:, 0].contiguous(), b[:, 1].contiguous(), b[:, 2].contiguous())


def test_non_deterministic_engine_takes_the_same_two_forms(tmp_path, golden_small, golden_na):
    """The float-atomic scatter path of the engine (deterministic=False) with `na`: both forms, both encoders, against the
    deterministic path's losses and gradient."""
    from idgrec_amd.engine import PropagationEngine

    b = torch.from_numpy(golden_na["batch"]).cuda()
    bt = tuple(b[:, c].contiguous() for c in range(3))
    for tag in TAGS:
        m, cfg, data = _model(tag, golden_na, tmp_path, golden_small)
        eng = m.engine()
        want_l = eng.loss_and_grad(*bt).clone()
        want_g = eng.grad.clone()
        loose = PropagationEngine(m.Graph if m.n_layers > 0 else None, data.num_users, data.num_items, m._storage.shape[1], m.n_layers,
                                  include_layer0=True, reg_lambda=m.reg_lambda, params=m._storage.clone(), deterministic=False)
        loose.na = eng.na
        got_l = loose.loss_and_grad(*bt)
        assert got_l.shape == want_l.shape == (_n_losses(tag),)
        np.testing.assert_allclose(got_l.cpu().numpy(), want_l.cpu().numpy(), rtol=1e-5)
        e = float((loose.grad - want_g).abs().max() / want_g.abs().max())
        print("%s: float-atomic path against the deterministic one: gradient %.2e of the largest entry" % (tag, e))
        assert e <= GRAD_TOL


def test_width_48_with_the_lightgcn_encoder_falls_back_to_autograd(tmp_path, golden_small, golden_na):
    m, cfg, data = _model("cscf_gcn", golden_na, tmp_path, golden_small, embedding_size=48)
    assert not m.fused_step_available()
    m2, _, _ = _model("ccf_mf", golden_na, tmp_path, golden_small, embedding_size=48)
    assert m2.fused_step_available()  # no propagation: every width the loss kernel takes
    b = torch.from_numpy(golden_na["batch"]).cuda()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 2
    sum(ll).backward()
    assert bool(torch.isfinite(m.user_embedding.weight.grad).all()) and float(m.user_embedding.weight.grad.abs().max()) > 0


# --------------------------------------------------------------------------------------- (e) end to end
@pytest.mark.parametrize("name,encoder,n_losses", [("LightCCF", "LightGCN", 3), ("LightCSCF", "LightGCN", 2)])
def test_trainer_end_to_end_on_small(name, encoder, n_losses, tmp_path, golden_small):
    import utility.utility_function.tools as tools

    cfg = _cfg(name, encoder=encoder, training_epochs=1, batch_size=256, test_batch_size=64, top_K="[5, 10]", interval=1)
    data = _small_data(tmp_path, golden_small, cfg)
    stream = io.StringIO()
    logger = logging.getLogger("na_e2e_" + name)
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models." + name).Trainer(None, cfg, data, torch.device("cuda"), logger)
    tr.train()
    assert tr.model.fused_step_available() and tr.model.n_fused_losses == n_losses
    lines = [ln.split("training loss:")[1] for ln in stream.getvalue().splitlines() if "training loss" in ln]
    assert len(lines) == 1
    nums = [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", lines[0])]
    assert len(nums) == 1 + n_losses, lines[0]
    assert np.isfinite(nums).all() and abs(nums[0] - sum(nums[1:])) < 1e-3 * max(1.0, abs(nums[0]))
