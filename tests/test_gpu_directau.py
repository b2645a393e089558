"""DirectAU on the GPU: the fused alignment / uniformity operator against float64 torch, the model against the reference's
goldens (both encoders), the fused training step against the autograd step, determinism and a full-size gradient check
at yelp2018 shape, and training end to end.
The operator's width list takes 192 from tests/widths.py (NF3_WIDTH): with it au_pair_mfma_kernel<3> is launched, and every NF = d / 64 = 1 .. 4 the source builds is held against float64.
Measured on an MI355X (59 tests, 7.4 s for the whole file; the 8 new cases 0.1 s together): d = 192 passes every B of the list
at the file's bounds (losses rtol 1e-5, gradients 1e-5 of the largest entry)."""
import importlib
import io
import logging
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(embedding_size=64, reg_lambda=0.0001, GCN_layer=3, batch_size=256, test_batch_size=64, training_epochs=3,
            interval=1, top_K="[5, 10]", early_stopping=10, learn_rate=0.001)


@pytest.fixture(scope="module")
def golden_au():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "directau_small.npz")))


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "DirectAU.txt"), "DirectAU")
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


def _ref64(fin, ego, users, pos, U, gamma, reg_lambda, same=False):
    """The reference's loss triple in float64 on the device: losses (3 floats) and d(sum)/d fin, d(sum)/d ego."""
    F = torch.nn.functional
    fin = fin.detach().double().requires_grad_(True)
    ego = fin if same else ego.detach().double().requires_grad_(True)
    B = users.shape[0]
    a = F.normalize(fin[users], dim=-1)
    b = F.normalize(fin[U + pos], dim=-1)
    align = (a - b).pow(2).sum(dim=1).mean()

    def unif(x):
        q = (x * x).sum(dim=1)
        D = (q[:, None] + q[None, :] - 2 * x @ x.T).clamp_min(0)
        iu = torch.triu_indices(B, B, 1, device=x.device)
        return torch.log(torch.exp(-2 * D[iu[0], iu[1]]).mean())

    uniform = gamma * (unif(a) + unif(b)) / 2 if B > 1 else torch.zeros((), dtype=torch.float64, device=fin.device)
    reg = reg_lambda * (0.5 * ego[users].pow(2).sum() / B + 0.5 * ego[U + pos].pow(2).sum() / B)
    (align + uniform + reg).backward()
    losses = [align.item(), uniform.item() if B > 1 else float("nan"), reg.item()]
    return losses, fin.grad, (None if same else ego.grad)


def _close_grad(mine, ref, tol=1e-5):
    mine, ref = mine.double().cpu().numpy(), ref.cpu().numpy()
    np.testing.assert_allclose(mine, ref, rtol=0, atol=tol * np.abs(ref).max())


# --------------------------------------------------------------------------------------- 1. the operator
@pytest.mark.parametrize("d", [32, 48, 64, 128, widths.NF3_WIDTH, 256])
@pytest.mark.parametrize("B", [1, 2, 3, 63, 64, 65, 1000, 2048])
def test_op_matches_float64_torch(B, d):
    from idgrec_amd import ops

    U, I = 700, 900
    gamma = 2.0 if (B + d) % 2 == 0 else 0.5
    gen = torch.Generator(device="cuda").manual_seed(B * 1000 + d)
    fin = torch.randn(U + I, d, device="cuda", generator=gen) * 0.3
    ego = torch.randn(U + I, d, device="cuda", generator=gen) * 0.1
    users = torch.randint(0, U, (B,), device="cuda", generator=gen)
    pos = torch.randint(0, I, (B,), device="cuda", generator=gen)
    if B >= 3:
        users[1], pos[2] = users[0], pos[0]  # duplicate ids (and a duplicated row pair)
    zero = B in (65, 1000) and d in (48, 64)
    if zero:
        fin[users[2]] = 0  # a row below the normalize() guard
    g_fin = torch.zeros_like(fin)
    g_ego = torch.zeros_like(ego)
    loss = ops.align_uniform_raw(fin, ego, users, pos, U, gamma, 1e-3, g_fin, g_ego)
    ref_loss, ref_gf, ref_ge = _ref64(fin, ego, users, pos, U, gamma, 1e-3)
    got = loss.cpu().numpy()
    np.testing.assert_allclose(got[[0, 2]], np.array(ref_loss)[[0, 2]], rtol=1e-5)
    if B == 1:
        assert np.isnan(got[1])  # torch.pdist of one row is empty: NaN, and no gradient from it (ref_* had gamma 0)
    else:
        np.testing.assert_allclose(got[1], ref_loss[1], rtol=1e-5)
    if zero:  # that row's gradient is scaled by 1 / 1e-12: compared on its own, the others against their own maximum
        zr = int(users[2])
        keep = torch.ones(U + I, dtype=torch.bool, device="cuda")
        keep[zr] = False
        _close_grad(g_fin[keep], ref_gf[keep])
        _close_grad(g_fin[zr], ref_gf[zr], tol=1e-4)
    else:
        _close_grad(g_fin, ref_gf)
    _close_grad(g_ego, ref_ge)
    # store mode: exactly the rows of users / num_users + pos are written, with the same values
    fill_f, fill_e = torch.full_like(fin, 7.0), torch.full_like(ego, 7.0)
    loss2 = ops.align_uniform_raw(fin, ego, users, pos, U, gamma, 1e-3, fill_f, fill_e, accumulate=False)
    rows = torch.zeros(U + I, dtype=torch.bool, device="cuda")
    rows[users] = True
    rows[U + pos] = True
    assert torch.equal(fill_f[rows], g_fin[rows]) and torch.equal(fill_e[rows], g_ego[rows])
    assert bool((fill_f[~rows] == 7).all()) and bool((fill_e[~rows] == 7).all())
    assert torch.equal(loss2.cpu(), loss.cpu()) or (B == 1 and np.array_equal(loss2.cpu().numpy(), got, equal_nan=True))


@pytest.mark.parametrize("d", [48, 64])
def test_op_autograd_and_same_panel(d):
    """align_uniform_loss under autograd (weighted sum of the three outputs) and the MF form (one panel)."""
    from idgrec_amd import ops

    U, I, B = 300, 400, 500
    gen = torch.Generator(device="cuda").manual_seed(d)
    fin = (torch.randn(U + I, d, device="cuda", generator=gen) * 0.3).requires_grad_(True)
    ego = (torch.randn(U + I, d, device="cuda", generator=gen) * 0.1).requires_grad_(True)
    users = torch.randint(0, U, (B,), device="cuda", generator=gen)
    pos = torch.randint(0, I, (B,), device="cuda", generator=gen)
    a, u, r = ops.align_uniform_loss(fin, ego, users, pos, U, 2.0, 1e-2)
    (0.5 * a + 2.0 * u + 3.0 * r).backward()
    f64, e64 = fin.detach().double().requires_grad_(True), ego.detach().double().requires_grad_(True)
    F = torch.nn.functional
    xa, xb = F.normalize(f64[users], dim=-1), F.normalize(f64[U + pos], dim=-1)

    def unif(x):
        return torch.log(torch.exp(-2 * torch.pdist(x).pow(2)).mean())

    ra = (xa - xb).pow(2).sum(1).mean()
    ru = 2.0 * (unif(xa) + unif(xb)) / 2
    rr = 1e-2 * (0.5 * e64[users].pow(2).sum() / B + 0.5 * e64[U + pos].pow(2).sum() / B)
    (0.5 * ra + 2.0 * ru + 3.0 * rr).backward()
    np.testing.assert_allclose([a.item(), u.item(), r.item()], [ra.item(), ru.item(), rr.item()], rtol=1e-5)
    _close_grad(fin.grad, f64.grad)
    _close_grad(ego.grad, e64.grad)
    # MF: final is ego, both gradients land in the one panel
    p = fin.detach().clone().requires_grad_(True)
    sum(ops.align_uniform_loss(p, p, users, pos, U, 2.0, 1e-2)).backward()
    ref_loss, ref_g, _ = _ref64(p, p, users, pos, U, 2.0, 1e-2, same=True)
    _close_grad(p.grad, ref_g)


# --------------------------------------------------------------------------------------- 2. reference goldens
@pytest.mark.parametrize("encoder", ["LightGCN", "MF"])
def test_model_matches_reference_goldens(encoder, tmp_path, golden_small, golden_au):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.DirectAU import DirectAU

    tag = encoder.lower()
    g = golden_au
    cfg = _cfg(encoder=encoder)
    data = _small_data(tmp_path, golden_small, cfg)
    tools.set_seed(2024)
    m = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
    b = torch.from_numpy(g["batch"]).cuda()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-5)
    sum(ll).backward()
    # (the reference's gradient is itself an fp32 computation: against it, the bound the operator meets against float64)
    for mine, ref in ((m.user_embedding.weight.grad, g[tag + "_grad_user"]), (m.item_embedding.weight.grad, g[tag + "_grad_item"])):
        np.testing.assert_allclose(mine.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
    m.eval()
    rating = m.get_rating_for_test(torch.from_numpy(g["rating_users"]).cuda())
    np.testing.assert_allclose(rating.cpu().numpy(), g[tag + "_rating"], rtol=1e-5, atol=1e-6)
    # the fused step, three batches, against the reference's own Adam trajectory
    m.train()
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    tools.set_seed(2024)
    m = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 3), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        assert m.fused_train_step(*bt, loss[i], opt)
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    # (Adam divides by sqrt(v): where a gradient is of the order of its own rounding error a last-place difference moves
    # the element visibly — the criterion of test_gpu_models' trajectory checks: 1e-4 relative on all but a handful of
    # elements, nowhere more than a tenth of one step's reach)
    for mine, ref in ((m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])):
        mine = mine.detach().cpu().numpy()
        off = ~np.isclose(mine, ref, rtol=1e-4, atol=1e-6)
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - ref).max() < 1e-4, np.abs(mine - ref).max()


# --------------------------------------------------------------------------------------- 3. fused step == autograd step
@pytest.mark.parametrize("encoder", ["LightGCN", "MF"])
def test_fused_step_equals_autograd_step(encoder, tmp_path, golden_small):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.DirectAU import DirectAU

    cfg = _cfg(encoder=encoder, **BASE)
    data = _small_data(tmp_path, golden_small, cfg)
    tri = torch.from_numpy(golden_small["sample1"][:5 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(5)]
    res = []
    for fused in (True, False):
        tools.set_seed(2024)
        model = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
        model.keep_fused_grad = True
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((3, 3), device="cuda")
        for i in range(3):
            if fused:
                assert model.fused_train_step(*bt[i], loss[i], opt)
            else:
                ll = model(*bt[i])
                loss[i] = torch.stack([x.detach() for x in ll])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
        res.append((loss.cpu().numpy(), model.user_embedding.weight.grad.cpu().numpy(), model._storage.cpu().numpy(),
                    opt.state[model.item_embedding.weight]["exp_avg_sq"].cpu().numpy()))
    (l_f, g_f, w_f, v_f), (l_a, g_a, w_a, v_a) = res
    np.testing.assert_allclose(l_f, l_a, rtol=2e-5)
    np.testing.assert_allclose(g_f, g_a, rtol=1e-3, atol=1e-5 * np.abs(g_a).max())
    np.testing.assert_allclose(w_f, w_a, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(v_f, v_a, rtol=2e-3, atol=1e-6 * np.abs(v_a).max())
    # one chain (Adam in the epilogue) == fused gradients + optimizer.step(), bit for bit, switching mid-run
    out = []
    for plan in ("TTTTT", "FTTFT"):
        tools.set_seed(2024)
        model = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
        model.keep_fused_grad = True
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((5, 3), device="cuda")
        for i, one_chain in enumerate(plan):
            if one_chain == "T":
                assert model.fused_train_step(*bt[i], loss[i], opt)
            else:
                model.fused_loss_and_grad(*bt[i], loss_out=loss[i])
                opt.step()
        st = opt.state[model.item_embedding.weight]
        assert st["step"] == 5
        out.append((model._storage.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), loss.clone(),
                    model.user_embedding.weight.grad.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------- 4./5. yelp2018 shape
@pytest.fixture(scope="module")
def yelp_data(tmp_path_factory):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    root = str(tmp_path_factory.mktemp("au_yelp"))
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = _cfg(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0")
    return data_loader.Data(os.path.join(root, "yelp2018"), cfg), cfg


def _yelp_batches(data, n, B=2048, seed=0):
    np.random.seed(seed)
    s = data.sample_data_to_train_all()
    tri = torch.from_numpy(s[:n * B]).cuda()
    return [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(n)]


def test_fused_training_is_bit_reproducible_at_yelp_shape(yelp_data):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.DirectAU import DirectAU

    data, cfg = yelp_data
    bt = _yelp_batches(data, 5)
    out = []
    for run in range(2):
        tools.set_seed(2024)
        model = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((5, 3), device="cuda")
        for i in range(5):
            if i + 1 < 5:
                model.prefetch_batch(*bt[i + 1])
            assert model.fused_train_step(*bt[i], loss[i], opt)
        st = opt.state[model.user_embedding.weight]
        out.append((model._storage.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), loss.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out[0][3]).all())


def test_full_size_gradient_against_float64_chain(yelp_data):
    import utility.utility_data.data_graph as data_graph
    import utility.utility_function.tools as tools
    from models.DirectAU import DirectAU

    data, cfg = yelp_data
    (u, p, n), = _yelp_batches(data, 1, seed=1)
    tools.set_seed(2024)
    model = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
    # (a trained-looking panel: the initial xavier rows are all of one scale)
    with torch.no_grad():
        model._storage.mul_(1 + torch.rand_like(model._storage))
    loss = model.fused_loss_and_grad(u, p, n).clone()
    grad = torch.cat([model.user_embedding.weight.grad, model.item_embedding.weight.grad]).clone()
    A = data_graph.sparse_adjacency_matrix(data).tocoo()
    A = torch.sparse_coo_tensor(np.vstack([A.row, A.col]), A.data.astype(np.float64), A.shape, device="cuda").coalesce()
    E0 = model._storage.detach().double().requires_grad_(True)
    layers, X = [E0], E0
    for _ in range(int(cfg["GCN_layer"])):
        X = torch.sparse.mm(A, X)
        layers.append(X)
    fin = torch.stack(layers, dim=1).mean(dim=1)
    F = torch.nn.functional
    U, B = data.num_users, u.shape[0]
    a, b = F.normalize(fin[u], dim=-1), F.normalize(fin[U + p], dim=-1)

    def unif(x):
        return torch.log(torch.exp(-2 * torch.pdist(x).pow(2)).mean())

    ra = (a - b).norm(dim=1).pow(2).mean()
    ru = float(cfg["gamma"]) * (unif(a) + unif(b)) / 2
    rr = float(cfg["reg_lambda"]) * (0.5 * E0[u].norm().pow(2) / B + 0.5 * E0[U + p].norm().pow(2) / B)
    (ra + ru + rr).backward()
    np.testing.assert_allclose(loss.cpu().numpy(), [ra.item(), ru.item(), rr.item()], rtol=1e-5)
    # At this shape fp32 arithmetic itself does not reach 1e-5 x max|g| everywhere: torch's own fp32 chain (torch.sparse.mm,
    # F.normalize, pdist) leaves 91 of 105,408 reached elements beyond it (3.2e-5 x max|g| at most).  So: 1e-5 x max|g|
    # on all but 1e-4 of the elements, and nowhere more than 5e-4 x max|g|
    mine, ref = grad.double().cpu().numpy(), E0.grad.cpu().numpy()
    err = np.abs(mine - ref) / np.abs(ref).max()
    assert (err > 1e-5).mean() < 1e-4, (err > 1e-5).sum()
    assert err.max() < 5e-4, err.max()


# --------------------------------------------------------------------------------------- 6. end to end
def _numbers(text):
    return [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", text)]


def _train(tmp_path, encoder, **kw):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    S.make_dataset(str(tmp_path), "medium", n_test=8)
    cfg = _cfg(encoder=encoder, dataset="medium", dataset_path=str(tmp_path) + "/", sparsity_test="0", interval=1,
               top_K="[20]", test_batch_size=2048, **kw)
    data = data_loader.Data(str(tmp_path / "medium"), cfg)
    stream = io.StringIO()
    logger = logging.getLogger("au_e2e_%s_%s" % (encoder, kw.get("embedding_size", 64)))
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models.DirectAU").Trainer(None, cfg, data, torch.device("cuda"), logger)
    tr.train()
    lines = stream.getvalue().splitlines()
    loss_lines = [ln.split("training loss:")[1] for ln in lines if "training loss" in ln]
    recalls = [_numbers(ln.split("Test recall:")[1].split("|")[0])[0] for ln in lines if "Test recall" in ln]
    return tr.model, loss_lines, recalls


@pytest.mark.parametrize("encoder", ["LightGCN", "MF"])
def test_trainer_end_to_end(encoder, tmp_path):
    model, loss_lines, recalls = _train(tmp_path, encoder, training_epochs=3, learn_rate=0.002, batch_size=1024)
    assert model.fused_step_available()
    assert len(loss_lines) == 3 and len(recalls) == 3
    totals, aligns = [], []
    for ln in loss_lines:
        assert re.fullmatch(r"\s*\S+ = \S+ \+ \S+ \+ \S+\s*", ln), ln
        t, a, u, r = _numbers(ln)
        assert abs(t - (a + u + r)) < 1e-4 and np.isfinite([a, u, r]).all()
        totals.append(t)
        aligns.append(a)
    assert totals[0] > totals[1] > totals[2], totals
    assert aligns[0] > aligns[1] > aligns[2], aligns
    # (Recall@20 on this synthetic shape does not rise within three epochs — measured 0.0120 / 0.0108 / 0.0103 with the
    # LightGCN encoder — so only its presence and range are checked)
    assert all(0 < x < 1 for x in recalls), recalls


def test_width_without_tiled_kernels_trains_through_autograd(tmp_path):
    model, loss_lines, recalls = _train(tmp_path, "LightGCN", training_epochs=2, embedding_size=48, learn_rate=0.002,
                                        batch_size=1024)
    assert not model.fused_step_available()
    totals = [_numbers(ln)[0] for ln in loss_lines]
    assert len(totals) == 2 and np.isfinite(totals).all() and totals[1] < totals[0]
    assert len(recalls) == 2
