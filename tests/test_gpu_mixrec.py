"""MixRec's fused contrastive kernels (idgrec_amd/csrc/idg_mixnce.hip), their differentiable wrapper (ops.mix_nce), the
engine (idgrec_amd/mixrec.py) and the plugin (models/MixRec.py) on the device.  The reference statement is
tests/mixrec_ref64.py, pinned to the reference's own numbers by tests/test_mixrec_host.py.

  (a) idg_mix_nce_f32 against float64 on generated rows: B in {1, 96, 127, 128, 129, 257} x d in {48, 64, 100, 256} x
      T in {0.2, 1.0}; the identity permutation and one with fixed points; beta in {0, 1, 1e-6, 0.5}; nu one-hot and with
      zeros; duplicate ids and all-distinct ids; a zero panel row as anchor, as negative and as permutation partner;
      upstream != 1; g_panel pre-filled (the gradient is ADDED);
      and B in {129, 257} over the widths of tests/widths.py (EVERY_NDT), which with the grid above launch every NDT =
      ceil(d / 32) = 1 .. 8 the source instantiates, the loss-only form of each included;
  (b) the loss-only call gives the bits of the gradient call's loss; two runs give identical bits;
  (c) ops.mix_nce under autograd is the raw call;
  (d) models.MixRec against the reference's fixture (tests/golden/mixrec_small.npz), both settings, the recorded draws
      injected: forward() losses, both table gradients, the rating; three fused steps against the reference's Adam
      trajectory; one fused step against forward() + autograd (loss, gradient, tables after Adam).

Tolerances.  Loss rtol 1e-5 and tables after Adam rtol 1e-4 / atol 1e-6 are the bounds tests/test_gpu_cgcl.py and
tests/test_gpu_bigcf.py apply to the same comparisons (the trajectory by test_gpu_bigcf.py's criterion: under 1e-3 of a
table's elements outside rtol 1e-4 / atol 1e-6 and none further than 1e-4 — Adam divides by sqrt(v), so where a gradient is
of the order of its own rounding a last-place difference moves the element visibly).  Gradients: the siblings' bound is
1e-5 of the largest entry; measured on the CPU (tests/test_mixrec_host.py prints it), the plain float32 torch composition of
the reference's expressions sits 5.5e-6 (`def`) and 5.4e-6 (`mid`) of the largest entry from tests/mixrec_ref64.py on the
fixture's inputs; the kernel is allowed twice that, GRAD_TOL = 1.1e-5 of the largest entry of the float64 gradient.  In (a) a
zero panel row's gradient carries F.normalize's 1 / 1e-12 (as under torch autograd) and is compared on its own scale, the
other rows on theirs.

Measured on an MI355X (84 tests, 34 s for the whole file): (a) gradients at most 0.76 of the bound (B = 96, d = 100, fixed
points, betas (0, 1); 0.36 over the size grid; 0.6 .. 0.7 with the identity permutation, where c = x and the positives' part
is almost all projected away), losses within 1.9e-6 relative at B = 1 and 2.9e-7 elsewhere; (d) forward() + backward() and
the fused step 6.1e-6 (`def`) and 3.6e-6 (`mid`) of the largest entry from the fixture, the fused step 3e-8 from forward() +
autograd; losses within 2e-7 of the fixture's; no trajectory element outside rtol 1e-4 / atol 1e-6 (largest difference
2.6e-6).
With the cases over every built width (104 tests, 5.1 s for the whole file without the first build; the 20 new
cases under 0.1 s together): gradients at most 0.33 of the bound (B = 129, d = 96), losses within 1.4e-7 relative, the loss-only
call's bits equal at every NDT."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import mixrec_ref64 as ref  # noqa: E402
from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
LOSS_RTOL, GRAD_TOL = 1e-5, 1.1e-5
PARAMS = ("user_embedding", "item_embedding")


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


# ================================================================================================== (a) the kernel vs float64
U_ROWS, I_ROWS = 45, 61


def _case(key, B, d, perm="random", betas=(0.37, 0.61), nu="dirichlet", distinct=False, zero=()):
    """Panel [U + I, d], ids with duplicates (or none), permutations, nu.  zero: roles whose panel row is zeroed — "anchor"
    (user 0 of the batch), "positive" (its positive), "negative" (negative 1), "partner" (the rows position 2 is mixed with)."""
    rng = _rng(key, B, d, perm, betas, nu, distinct, zero)
    U, I = (max(U_ROWS, B), max(I_ROWS, 2 * B)) if distinct else (U_ROWS, I_ROWS)
    panel = (rng.standard_normal((U + I, d)) * 0.3).astype(np.float32)
    if distinct:
        users, items = rng.permutation(U)[:B], rng.permutation(I)[:2 * B]
        pos, neg = items[:B], items[B:]
    else:
        users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    if perm == "identity":
        up, ip = np.arange(B), np.arange(B)
    else:
        up, ip = rng.permutation(B), rng.permutation(B)
        if perm == "fixed points" and B > 3:
            for p in (up, ip):
                for i in (0, 3):  # two fixed points each; still permutations
                    j = int(np.nonzero(p == i)[0][0])
                    p[j], p[i] = p[i], i
    if nu == "one-hot":
        w = np.zeros(B)
        w[B // 2] = 1
    else:
        w = rng.dirichlet([0.5] * B)
        if nu == "zeros" and B > 2:
            w[::2] = 0
            w /= w.sum()
    for role in zero:
        if role == "anchor":
            panel[users[0]] = 0
        elif role == "positive":
            panel[U + pos[0]] = 0
        elif role == "negative":
            panel[U + neg[1 % B]] = 0
        elif role == "partner":
            panel[users[up[2 % B]]] = 0
            panel[U + pos[ip[2 % B]]] = 0
            panel[U + neg[ip[2 % B]]] = 0
    ids = tuple(dev(np.asarray(a, dtype=np.int64)) for a in (users, pos, neg))
    draws = (float(betas[0]), float(betas[1]), dev(w.astype(np.float32)), dev(up.astype(np.int64)), dev(ip.astype(np.int64)))
    return dev(panel), U, ids, draws


def _run(ops, panel, U, ids, draws, t, w, upstream=None, base=None, grads=True):
    ub, ib, nu, up, ip = draws
    g = None
    if grads:
        g = torch.zeros_like(panel) if base is None else base.clone()
    up_dev = None if upstream is None else torch.tensor(upstream, dtype=F32, device="cuda")
    loss = ops.mix_nce_raw(panel, U, *ids, up, ip, nu, ub, ib, t, w, upstream=up_dev, g_panel=g).clone()
    return loss, g


def _check(tag, ops, panel, U, ids, draws, t, w=1.1, upstream=None, base=None):
    loss, g = _run(ops, panel, U, ids, draws, t, w, upstream, base)
    # the kernel takes both betas as float32: the reference is given the same numbers
    d64 = (float(np.float32(draws[0])), float(np.float32(draws[1]))) + draws[2:]
    l64, g64 = ref.panel_terms(panel, U, *ids, d64, t, float(np.float32(w)), upstream=upstream)
    assert torch.isfinite(loss).all() and torch.isfinite(g).all(), tag
    assert torch.equal(loss == 0, l64 == 0), tag + ": an entry whose weight is zero"  # (item_beta = 1: loss[0] is exactly 0)
    e_loss = float(((loss.double() - l64).abs() / l64.abs().clamp_min(1e-300)).max())
    got = g.double() - (0 if base is None else base.double())
    zero_rows = panel.abs().sum(dim=1) == 0
    worst = 0.0
    for name, rows in (("rows", ~zero_rows), ("zero rows", zero_rows)):
        if not bool(rows.any()):
            continue
        if float(g64[rows].abs().max()) == 0:
            assert float(got[rows].abs().max()) == 0, "%s: gradient at %s that take none" % (tag, name)
            continue
        scale = float(g64[rows].abs().max())
        tol = GRAD_TOL + (2.0 ** -23 * float(base.abs().max()) / scale if base is not None else 0)  # (the addition's own rounding)
        e = float((got[rows] - g64[rows]).abs().max()) / scale
        worst = max(worst, e / tol)
        assert e <= tol, "%s: gradient (%s) %.3e of the largest entry, bound %.3e" % (tag, name, e, tol)
    touched = torch.zeros(panel.shape[0], dtype=torch.bool, device="cuda")
    touched[ids[0]] = True
    touched[U + ids[1]] = True
    touched[U + ids[2]] = True
    assert float(got[~touched].abs().max() if bool((~touched).any()) else 0) == 0, tag + ": rows outside the batch were written"
    print("  %-70s loss %.2e  gradient %.2f of the bound" % (tag, e_loss, worst))
    assert e_loss <= LOSS_RTOL, "%s: loss %.3e relative" % (tag, e_loss)


@pytest.mark.parametrize("t", [0.2, 1.0])
@pytest.mark.parametrize("d", [48, 64, 100, 256])
@pytest.mark.parametrize("B", [1, 96, 127, 128, 129, 257])
def test_kernel_vs_float64_over_sizes(ops, B, d, t):
    panel, U, ids, draws = _case("sizes", B, d)
    _check("B=%d d=%d T=%g" % (B, d, t), ops, panel, U, ids, draws, t)


@pytest.mark.parametrize("d", widths.EVERY_NDT)
@pytest.mark.parametrize("B", widths.B_TILES)
def test_kernel_vs_float64_over_every_built_width(ops, B, d):
    """Every NDT = ceil(d / 32) the source instantiates, with gradients (MODE_SUMS_ACC and the table pass) and, at B = 129,
    through the loss-only call (MODE_SUMS) too: the bits of the gradient call's loss."""
    panel, U, ids, draws = _case("widths", B, d)
    _check("B=%d d=%d (NDT %d) T=0.2" % (B, d, widths.ndt(d)), ops, panel, U, ids, draws, 0.2)
    if B == 129:
        l1, _ = _run(ops, panel, U, ids, draws, 0.2, 1.1)
        l0, _ = _run(ops, panel, U, ids, draws, 0.2, 1.1, grads=False)
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), "the loss-only call gives other bits"


@pytest.mark.parametrize("perm", ["identity", "fixed points"])
@pytest.mark.parametrize("betas", [(0.0, 1.0), (1.0, 0.0), (1e-6, 1e-6), (0.5, 0.5)])
def test_kernel_vs_float64_permutations_and_weights(ops, perm, betas):
    for B, d in ((129, 64), (96, 100)):
        panel, U, ids, draws = _case("perm", B, d, perm=perm, betas=betas)
        _check("B=%d d=%d %s betas=%s" % (B, d, perm, betas), ops, panel, U, ids, draws, 0.2)


@pytest.mark.parametrize("nu", ["one-hot", "zeros"])
@pytest.mark.parametrize("distinct", [False, True])
def test_kernel_vs_float64_nu_and_duplicates(ops, nu, distinct):
    for B, d in ((129, 64), (257, 48)):
        panel, U, ids, draws = _case("nu", B, d, nu=nu, distinct=distinct)
        if not distinct:
            assert all(len(set(i.tolist())) < B for i in ids)  # duplicate users, positives and negatives
        _check("B=%d d=%d nu=%s distinct=%s" % (B, d, nu, distinct), ops, panel, U, ids, draws, 0.2)


@pytest.mark.parametrize("zero", [("anchor",), ("positive",), ("negative",), ("partner",), ("anchor", "positive", "negative", "partner")])
@pytest.mark.parametrize("perm", ["random", "identity"])
def test_kernel_vs_float64_zero_rows(ops, zero, perm):
    for B, d in ((129, 64), (96, 48)):
        panel, U, ids, draws = _case("zero", B, d, perm=perm, zero=zero)
        assert bool((panel.abs().sum(dim=1) == 0).any())
        _check("B=%d d=%d %s zero=%s" % (B, d, perm, "+".join(zero)), ops, panel, U, ids, draws, 0.2)


@pytest.mark.parametrize("B,d", [(129, 64), (257, 100), (1, 64)])
def test_kernel_upstream_and_prefilled_gradient(ops, B, d):
    panel, U, ids, draws = _case("upstream", B, d)
    _check("B=%d d=%d upstream" % (B, d), ops, panel, U, ids, draws, 0.2, upstream=(0.25, 3.0))
    base = dev((_rng("base", B, d).standard_normal(tuple(panel.shape)) * 1e-3).astype(np.float32))
    _check("B=%d d=%d added into a filled panel" % (B, d), ops, panel, U, ids, draws, 0.2, upstream=(1.5, 0.5), base=base)


# ============================================================================================== (b) loss-only, run to run
@pytest.mark.parametrize("B,d", [(1, 64), (129, 64), (257, 100), (2048, 64)])
def test_loss_only_call_and_second_run_give_the_same_bits(ops, B, d):
    panel, U, ids, draws = _case("bits", B, d)
    l1, g1 = _run(ops, panel, U, ids, draws, 0.2, 1.1)
    l0, _ = _run(ops, panel, U, ids, draws, 0.2, 1.1, grads=False)
    l2, g2 = _run(ops, panel, U, ids, draws, 0.2, 1.1)
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), "the loss-only call gives other bits"
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))


# ======================================================================================================== (c) under autograd
def test_autograd_is_the_raw_call(ops):
    panel, U, ids, draws = _case("autograd", 129, 64)
    ub, ib, nu, up, ip = draws
    x = panel.clone().requires_grad_(True)
    l0, l1 = ops.mix_nce(x, U, *ids, up, ip, nu, ub, ib, 0.2, 1.1)
    (0.25 * l0 + 3.0 * l1).backward()
    loss, g = _run(ops, panel, U, ids, draws, 0.2, 1.1, upstream=(0.25, 3.0))
    assert torch.equal(torch.stack([l0, l1]).detach(), loss) and torch.equal(x.grad, g)


# ================================================================================================================ (d) the plugin
@pytest.fixture(scope="module")
def golden_mixrec():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mixrec_small.npz"), allow_pickle=False))


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "MixRec.txt"), "MixRec")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _model(tmp_path, golden_small, g, tag):
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools
    from models.MixRec import MixRec

    alpha, beta, gamma = g[tag + "_abg"].tolist()
    cfg = _cfg(GCN_layer=2, alpha=alpha, beta=beta, gamma=gamma)
    d = tmp_path / "small"
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(golden_small["train_txt"].tobytes())
    (d / "test.txt").write_bytes(golden_small["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(d), cfg)
    tools.set_seed(2024)
    m = MixRec(cfg, data, torch.device("cuda")).to("cuda")
    prm = {p: getattr(m, p).weight for p in PARAMS}
    for p in PARAMS:  # same torch RNG order as the reference's constructor
        assert np.array_equal(prm[p].detach().cpu().numpy(), g["init_" + p]), p
    return cfg, m, prm


def _draws(g, prefix):
    return (float(g[prefix + "_betas"][0]), float(g[prefix + "_betas"][1]), torch.from_numpy(g[prefix + "_nu"]),
            torch.from_numpy(g[prefix + "_user_perm"]), torch.from_numpy(g[prefix + "_item_perm"]))


def _grad_check(what, mine, want):
    e = float(np.abs(mine - want).max() / np.abs(want).max())
    print("  %-60s %.3e of the largest entry (bound %.1e)" % (what, e, GRAD_TOL))
    assert e <= GRAD_TOL, (what, e)


def _tables_check(what, mine, want):
    off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
    print("  %-60s outside rtol 1e-4 / atol 1e-6: %.3g of the elements, largest difference %.3g" % (what, off.mean(), np.abs(mine - want).max()))
    assert off.mean() < 1e-3 and np.abs(mine - want).max() < 1e-4, (what, off.mean(), np.abs(mine - want).max())


@pytest.mark.parametrize("tag", ["def", "mid"])
def test_model_forward_matches_the_fixture(ops, tag, tmp_path, golden_small, golden_mixrec):
    g = golden_mixrec
    cfg, m, prm = _model(tmp_path, golden_small, g, tag)
    assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
    b = torch.from_numpy(g["batch"]).cuda()
    m.mix_source = lambda: _draws(g, tag)
    m.zero_grad()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 4
    sum(ll).backward()
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=LOSS_RTOL)
    mine = np.concatenate([prm[p].grad.cpu().numpy() for p in PARAMS])
    want = np.concatenate([g["%s_grad_%s" % (tag, p)] for p in PARAMS])
    _grad_check(tag + " table gradients of forward() + backward()", mine, want)
    m.eval()
    users = torch.from_numpy(g["rating_users"]).cuda()
    np.testing.assert_allclose(m.get_rating_for_test(users).cpu().numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    assert m.topk_for_test(users, 10).shape == (32, 10)
    # without a source the plugin draws for itself, from numpy's and torch's global generators
    m.train()
    m.mix_source = None
    np.random.seed(5)
    torch.manual_seed(5)
    l1 = [x.item() for x in m(b[:, 0], b[:, 1], b[:, 2])]
    l2 = [x.item() for x in m(b[:, 0], b[:, 1], b[:, 2])]
    np.random.seed(5)
    torch.manual_seed(5)
    l3 = [x.item() for x in m(b[:, 0], b[:, 1], b[:, 2])]
    assert np.isfinite(l1).all() and l1 != l2 and l1 == l3


@pytest.mark.parametrize("tag", ["def", "mid"])
def test_model_fused_steps_match_the_fixtures_trajectory(ops, tag, tmp_path, golden_small, golden_mixrec):
    g = golden_mixrec
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    cfg, m, prm = _model(tmp_path, golden_small, g, tag)
    assert m.fused_step_available()
    seq = iter([_draws(g, "%s_traj%d" % (tag, i)) for i in range(3)])
    m.mix_source = lambda: next(seq)
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 4), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=LOSS_RTOL)
    for p in PARAMS:
        _tables_check("%s trajectory %s" % (tag, p), prm[p].detach().cpu().numpy(), g["%s_traj_%s" % (tag, p)])
    assert all(int(opt.state[q]["step"]) == 3 for q in m.parameters())


@pytest.mark.parametrize("tag", ["def", "mid"])
def test_fused_step_matches_forward_and_autograd(ops, tag, tmp_path, golden_small, golden_mixrec):
    g = golden_mixrec
    b = tuple(torch.from_numpy(g["batch"][:, c].copy()).cuda() for c in range(3))
    draws = _draws(g, tag)
    cfg, m, prm = _model(tmp_path, golden_small, g, tag)
    m.mix_source = lambda: draws
    # forward() + autograd + the same Adam kernel
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    ll = m(*b)
    opt.zero_grad()
    sum(ll).backward()
    grad_a = np.concatenate([prm[p].grad.cpu().numpy() for p in PARAMS])
    opt.step()
    loss_a = np.array([x.item() for x in ll])
    tables_a = np.concatenate([prm[p].detach().cpu().numpy() for p in PARAMS])
    # the fused step from the same initial tables
    cfg, m2, prm2 = _model(tmp_path, golden_small, g, tag)
    m2.mix_source = lambda: draws
    opt2 = ops.Adam(m2.parameters(), lr=float(cfg["learn_rate"]))
    eng = m2.mixrec_engine()
    eng.store_grad = True
    loss_f = torch.zeros(4, device="cuda")
    assert m2.fused_train_step(*b, loss_f, opt2)
    np.testing.assert_allclose(loss_f.cpu().numpy(), loss_a, rtol=LOSS_RTOL)
    np.testing.assert_allclose(loss_f.cpu().numpy(), g[tag + "_loss"], rtol=LOSS_RTOL)
    _grad_check(tag + " fused gradient vs forward() + autograd", eng.GRAD.cpu().numpy(), grad_a)
    want = np.concatenate([g["%s_grad_%s" % (tag, p)] for p in PARAMS])
    _grad_check(tag + " fused gradient vs the fixture", eng.GRAD.cpu().numpy(), want)
    tables_f = np.concatenate([prm2[p].detach().cpu().numpy() for p in PARAMS])
    _tables_check(tag + " tables after Adam, fused vs forward() + autograd", tables_f, tables_a)
    assert not np.array_equal(tables_f, np.concatenate([g["init_" + p] for p in PARAMS]))
