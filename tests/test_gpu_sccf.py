"""SCCF on the GPU: idg_sccf_loss_f32 against the float64 statement (tests/sccf_ref64.py) across its tile edges, widths and
temperatures; the same bits with and without gradients, with a plan built ahead, and run to run; ops.sccf_loss under
autograd; models.SCCF against the reference's fixture (both encoders), its fused step against the reference's Adam
trajectory and against forward() + autograd; training end to end.

Tolerances.  Losses rtol 1e-5, tables after Adam rtol 1e-4 / atol 1e-6 (the siblings' bounds); the trajectory by
tests/test_gpu_bigcf.py's criterion (under 1e-3 of a table's elements outside that band, none further than 1e-4 — which the
reference's own float32 run meets: tests/test_sccf_host.py).  Gradients: GRAD_TOL = 4.3e-6 of the largest entry of the
float64 gradient = twice the worst float32 yardstick tests/test_sccf_host.py measures over grid (a) with the cases riding on
it (tests/sccf_ref64.py: RIDERS) and the fixture — 2.11e-6, one user repeated 129 times at T = 1 — rounded up to two digits;
tighter than the siblings' 1e-5, which would otherwise cap it.  A zero panel row's own gradient
carries normalize()'s 1e12 and is compared on its own scale, at the siblings' 1e-4.
The cases over the widths of tests/widths.py (EVERY_NDT at B = 129 and 257, T = 0.1), which with grid (a) launch every NDT =
ceil(d / 32) = 1 .. 8 the source instantiates, take GRAD_TOL unchanged: their worst float32 yardstick is 7.7e-7 (B = 257,
d = 32; tests/test_sccf_host.py).

Measured on an MI355X (70 tests, 32 s).  The kernel's gradients over grid (a): at most 8.0e-7 of the largest entry = 0.19 of
GRAD_TOL (B = 257, d = 48, T = 0.1), 1.2e-7 ... 3.2e-7 at T = 1; the riders: all-distinct ids at most 2.9e-7, zero rows 4.4e-7, one
repeated user 5.3e-7 (B = 96), 6.9e-7 (B = 257) and 1.35e-6 = 0.31 of GRAD_TOL at B = 129, d = 48, T = 1 — the case that set the
yardstick.  (With the 1/Z factor rounded to float and the row sums as single 128-term fp32 chains that case sat at 5.2e-6 and
failed; the factor is now kept in double and every chain has 32 terms.)  Losses within 6.2e-7 relative at B = 1 (d = 256), 1.8e-7
elsewhere.  The plugin's .grad against the fixture: 8.3e-7 (`mf`), 5.8e-7 (`gcn`); three fused steps: no element outside rtol
1e-4 / atol 1e-6, 3.0e-8 (`mf`) and 5.2e-6 (`gcn`) off at most; the fused step's gradient equals forward() + autograd's bit for
bit (the same kernels in the same order).
With the cases over every built width (90 tests, 4.2 s; the 20 new cases under 0.1 s together): gradients at most 1.08e-6 of
the largest entry = 0.25 of GRAD_TOL (B = 129, d = 32), 3.0e-7 at B = 257, d = 200; losses within 6.6e-8 relative.
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

from tests import sccf_ref64 as ref  # noqa: E402
from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 4.3e-6
TAGS = {"mf": "MF", "gcn": "LightGCN"}
WORST = {"loss": 0.0, "grad": 0.0}


@pytest.fixture(scope="module")
def golden_sccf():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "sccf_small.npz")))


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "SCCF.txt"), "SCCF")
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


def _grad_err(mine, ref64, rows=None):
    mine, ref64 = mine.double().cpu(), ref64.double().cpu()
    if rows is not None:
        mine, ref64 = mine[rows], ref64[rows]
    return float((mine - ref64).abs().max() / ref64.abs().max())


def _check(loss, g, panel, U, users, pos, t, upstream=None, skip_rows=None, what=""):
    """Losses at rtol 1e-5 and the gradient at GRAD_TOL against the float64 literal form; prints every figure first."""
    l64, g64 = ref.panel_terms(panel.cpu(), U, users.cpu(), pos.cpu(), t, upstream=upstream)
    e_l = float(((loss.double().cpu() - l64) / l64).abs().max())
    keep = torch.ones(panel.shape[0], dtype=torch.bool)
    if skip_rows:
        keep[list(skip_rows)] = False
    e_g = _grad_err(g, g64, keep)
    WORST["loss"], WORST["grad"] = max(WORST["loss"], e_l), max(WORST["grad"], e_g)
    print("%s: losses %.2e (relative), gradient %.2e of the largest entry = %.2f of GRAD_TOL" % (what, e_l, e_g, e_g / GRAD_TOL))
    assert e_l <= 1e-5, (what, e_l)
    assert e_g <= GRAD_TOL, (what, e_g)
    for r in skip_rows or ():
        assert _grad_err(g[r], g64[r]) <= 1e-4, (what, r)
    return l64, g64


def _up(pair):
    return None if pair is None else torch.tensor(pair, dtype=torch.float32, device="cuda")


# --------------------------------------------------------------------------------------- (a) the grid
@pytest.mark.parametrize("t", ref.GRID_T)
@pytest.mark.parametrize("d", ref.GRID_D)
@pytest.mark.parametrize("B", ref.GRID_B)
def test_op_matches_float64_statement(B, d, t):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, ref.grid_seed(B, d, t), device="cuda")
    pair = ref.grid_upstream(B)
    g = torch.zeros_like(panel)
    loss = ops.sccf_loss_raw(panel, users, pos, U, t, g, upstream=_up(pair))
    _check(loss, g, panel, U, users, pos, t, upstream=pair, what="B=%d d=%d T=%g" % (B, d, t))
    if B >= 96:
        assert int(torch.unique(users).numel()) < B and int(torch.unique(pos).numel()) < B  # 45 / 61 rows: ids repeat


@pytest.mark.parametrize("d", widths.EVERY_NDT)
@pytest.mark.parametrize("B", ref.WIDTH_B)
def test_op_matches_float64_statement_over_every_built_width(B, d):
    """Every NDT = ceil(d / 32) the source instantiates, with gradients and, at B = 129, through the loss-only call too (the
    same bits).  GRAD_TOL unchanged: tests/test_sccf_host.py measures the float32 yardstick of these cases below half of it."""
    from idgrec_amd import ops

    t = ref.WIDTH_T
    panel, users, pos, U = ref.case_inputs(B, d, ref.width_seed(B, d), device="cuda")
    pair = ref.grid_upstream(B)
    g = torch.zeros_like(panel)
    loss = ops.sccf_loss_raw(panel, users, pos, U, t, g, upstream=_up(pair)).clone()
    _check(loss, g, panel, U, users, pos, t, upstream=pair, what="widths B=%d d=%d (NDT %d) T=%g" % (B, d, widths.ndt(d), t))
    if B == 129:
        l0 = ops.sccf_loss_raw(panel, users, pos, U, t).clone()
        assert torch.equal(l0, loss)  # the loss alone: the same bits as with gradients


def _riders(*forms):
    return [c for c in ref.RIDERS if c[0] in forms]


@pytest.mark.parametrize("form,B,d,t,seed", _riders("distinct", "one_user"))
def test_op_on_distinct_ids_and_one_repeated_user(form, B, d, t, seed):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, seed, device="cuda", form=form)
    assert int(torch.unique(users).numel()) == (B if form == "distinct" else 1)
    g = torch.zeros_like(panel)
    loss = ops.sccf_loss_raw(panel, users, pos, U, t, g)
    _check(loss, g, panel, U, users, pos, t, what="%s B=%d d=%d T=%g" % (form, B, d, t))


@pytest.mark.parametrize("form,B,d,t,seed", _riders("zero_rows"))
def test_op_with_a_zero_row_as_user_and_as_positive(form, B, d, t, seed):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, seed, device="cuda", form=form)
    zu, zp = ref.zero_rows_of(users, pos, U)
    assert float(panel[zu].abs().max()) == 0 and float(panel[zp].abs().max()) == 0
    g = torch.zeros_like(panel)
    loss = ops.sccf_loss_raw(panel, users, pos, U, t, g)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
    _check(loss, g, panel, U, users, pos, t, skip_rows=(zu, zp), what="zero rows B=%d d=%d T=%g" % (B, d, t))


@pytest.mark.parametrize("form,B,d,t,seed", _riders("random"))
def test_op_accumulates_and_stores(form, B, d, t, seed):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, seed, device="cuda")
    n = panel.shape[0]
    g = torch.zeros_like(panel)
    loss = ops.sccf_loss_raw(panel, users, pos, U, t, g)
    rows = torch.zeros(n, dtype=torch.bool, device="cuda")
    rows[users] = True
    rows[U + pos] = True
    if B == 127:  # leave rows outside the batch
        assert not bool(rows.all())
    # accumulate = 1 into a pre-filled panel: added
    gen = torch.Generator(device="cuda").manual_seed(B)
    fill = torch.randn(panel.shape, device="cuda", generator=gen) * float(g.abs().max())
    acc = fill.clone()
    ops.sccf_loss_raw(panel, users, pos, U, t, acc)
    assert torch.equal(acc[rows], (fill + g)[rows]) and torch.equal(acc[~rows], fill[~rows])
    # accumulate = 0 into a sentinel: the batch's rows hold the gradient, every other element keeps its bits; g_ego's rows of
    # the batch are exactly 0, the others untouched
    sent = float.fromhex("0x1.234566p+3")
    st, eg = torch.full_like(panel, sent), torch.full_like(panel, sent)
    loss2 = ops.sccf_loss_raw(panel, users, pos, U, t, st, eg, accumulate=False)
    assert torch.equal(st[rows], g[rows]) and bool((st[~rows] == sent).all())
    assert bool((eg[rows] == 0).all()) and bool((eg[~rows] == sent).all())
    assert torch.equal(loss2, loss)
    # accumulate = 1 leaves g_ego alone
    eg2 = torch.full_like(panel, sent)
    ops.sccf_loss_raw(panel, users, pos, U, t, torch.zeros_like(panel), eg2, accumulate=True)
    assert bool((eg2 == sent).all())
    _check(loss, g, panel, U, users, pos, t, what="store / accumulate B=%d d=%d T=%g" % (B, d, t))


# --------------------------------------------------------------------------------------- (b) the same bits
@pytest.mark.parametrize("B,d,t", [(1, 64, 0.1), (129, 100, 0.1), (257, 256, 1.0)])
def test_same_bits_loss_only_planned_and_rerun(B, d, t):
    from idgrec_amd import ops

    panel, users, pos, U = ref.case_inputs(B, d, 7 * B + d, device="cuda")
    g1, g2, g3 = (torch.zeros_like(panel) for _ in range(3))
    l1 = ops.sccf_loss_raw(panel, users, pos, U, t, g1).clone()
    l0 = ops.sccf_loss_raw(panel, users, pos, U, t).clone()
    assert torch.equal(l0, l1)  # the loss alone: the same bits as with gradients
    l2 = ops.sccf_loss_raw(panel, users, pos, U, t, g2, ws=ops.sccf_workspace(B, d, "cuda")).clone()
    assert torch.equal(l2, l1) and torch.equal(g2, g1)  # run to run (and in a fresh workspace)
    plan = ops.bpr_workspace(B, d, "cuda")
    ops.bpr_plan_raw(users, pos, pos, U, panel.shape[0], d, ws=plan)
    l3 = ops.sccf_loss_raw(panel, users, pos, U, t, g3, plan_ws=plan).clone()
    l4 = ops.sccf_loss_raw(panel, users, pos, U, t, plan_ws=plan).clone()
    assert torch.equal(l3, l1) and torch.equal(g3, g1) and torch.equal(l4, l1)


# --------------------------------------------------------------------------------------- (c) autograd
@pytest.mark.parametrize("d", [48, 64])
def test_op_under_autograd_equals_the_raw_call(d):
    from idgrec_amd import ops

    B, t = 129, 0.2
    panel, users, pos, U = ref.case_inputs(B, d, 5 * d, device="cuda")
    p = panel.clone().requires_grad_(True)
    neg_up, down = ops.sccf_loss(p, users, pos, U, t)
    (0.7 * neg_up - 1.3 * down).backward()
    g = torch.zeros_like(panel)
    loss = ops.sccf_loss_raw(panel, users, pos, U, t, g, upstream=_up((0.7, -1.3)))
    assert torch.equal(torch.stack([neg_up.detach(), down.detach()]), loss) and torch.equal(p.grad, g)
    _check(loss, g, panel, U, users, pos, t, upstream=(0.7, -1.3), what="autograd d=%d" % d)


# --------------------------------------------------------------------------------------- (d) the model
def _model(tag, g, tmp_path, golden_small, **kw):
    import utility.utility_function.tools as tools
    from models.SCCF import SCCF

    t, layers, lr = g[tag + "_hyper"].tolist()
    cfg = _cfg(encoder=TAGS[tag], temperature=t, GCN_layer=int(layers), learn_rate=lr, **kw)
    data = _small_data(tmp_path, golden_small, cfg)
    tools.set_seed(2024)
    return SCCF(cfg, data, torch.device("cuda")).to("cuda"), cfg, data


@pytest.mark.parametrize("tag", list(TAGS))
def test_model_matches_reference_fixture(tag, tmp_path, golden_small, golden_sccf):
    from idgrec_amd import ops

    g = golden_sccf
    m, cfg, data = _model(tag, g, tmp_path, golden_small)
    np.testing.assert_array_equal(m.user_embedding.weight.detach().cpu().numpy(), g["init_user_embedding"])
    b = torch.from_numpy(g["batch"]).cuda()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 2
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-5)
    sum(ll).backward()
    for p in ("user_embedding", "item_embedding"):
        want = g["%s_grad_%s" % (tag, p)]
        e = float(np.abs(getattr(m, p).weight.grad.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print("%s %s.grad: %.2e of the largest entry = %.2f of GRAD_TOL" % (tag, p, e, e / GRAD_TOL))
        assert e <= GRAD_TOL, (p, e)
    m.eval()
    rating = m.get_rating_for_test(torch.from_numpy(g["rating_users"]).cuda())
    np.testing.assert_allclose(rating.cpu().numpy(), g[tag + "_rating"], rtol=1e-5, atol=1e-6)
    # three fused steps against the reference's own Adam trajectory
    m, cfg, data = _model(tag, g, tmp_path, golden_small)
    assert m.fused_step_available()
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 2), device="cuda")
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


@pytest.mark.parametrize("tag", list(TAGS))
def test_fused_step_equals_autograd_step(tag, tmp_path, golden_small, golden_sccf):
    from idgrec_amd import ops

    g = golden_sccf
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    bt = tuple(tri[:256, c].contiguous() for c in range(3))
    res = []
    for fused in (True, False):
        m, cfg, data = _model(tag, g, tmp_path, golden_small)
        m.keep_fused_grad = True
        opt = ops.Adam(m.parameters(), lr=0.001)
        loss = torch.zeros(2, device="cuda")
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


def test_engine_refuses_au_and_sccf_together(tmp_path, golden_small, golden_sccf):
    m, cfg, data = _model("mf", golden_sccf, tmp_path, golden_small)
    eng = m.engine()
    assert eng.sccf == (m.temperature,) and eng.au is None
    eng.au = (2.0,)
    b = torch.from_numpy(golden_sccf["batch"]).cuda()
    with pytest.raises(ValueError, match="au and sccf"):
        eng.loss_and_grad(b[:, 0].contiguous(), b[:, 1].contiguous(), b[:, 2].contiguous())


def test_width_48_with_the_lightgcn_encoder_falls_back_to_autograd(tmp_path, golden_small, golden_sccf):
    m, cfg, data = _model("gcn", golden_sccf, tmp_path, golden_small, embedding_size=48)
    assert not m.fused_step_available()
    m2, _, _ = _model("mf", golden_sccf, tmp_path, golden_small, embedding_size=48)
    assert m2.fused_step_available()  # no propagation: every width the loss kernel takes
    b = torch.from_numpy(golden_sccf["batch"]).cuda()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    sum(ll).backward()
    assert bool(torch.isfinite(m.user_embedding.weight.grad).all()) and float(m.user_embedding.weight.grad.abs().max()) > 0


# --------------------------------------------------------------------------------------- (e) end to end
def test_trainer_end_to_end_on_small(tmp_path, golden_small):
    import utility.utility_function.tools as tools

    cfg = _cfg(encoder="MF", training_epochs=1, batch_size=256, test_batch_size=64, top_K="[5, 10]", interval=1)
    data = _small_data(tmp_path, golden_small, cfg)
    stream = io.StringIO()
    logger = logging.getLogger("sccf_e2e")
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models.SCCF").Trainer(None, cfg, data, torch.device("cuda"), logger)
    tr.train()
    assert tr.model.fused_step_available()
    lines = [ln.split("training loss:")[1] for ln in stream.getvalue().splitlines() if "training loss" in ln]
    assert len(lines) == 1
    assert re.fullmatch(r"\s*\S+ = \S+ \+ \S+\s*", lines[0]), lines[0]
    total, a, b = [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", lines[0])]
    assert np.isfinite([total, a, b]).all() and abs(total - (a + b)) < 1e-4
