"""CGCL on the GPU: the full-table contrastive operator against float64 torch (every width path, tile remainders, the
regime where the +1e-7 guard decides), its autograd form, the model against the reference's goldens in two settings, the
fused training step against the autograd step, determinism, the memory condition (no [B, N] buffer), and training end to
end."""
import importlib
import io
import logging
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRONG = dict(ssl_lambda_alpha=0.1, ssl_lambda_beta=0.1, ssl_lambda_gamma=0.1, alpha=0.3, beta=0.6, gamma=0.8)


@pytest.fixture(scope="module")
def golden_cgcl():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "cgcl_small.npz")))


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "CGCL.txt"), "CGCL")
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


def _ref64(table_panel, row0, N, query_panels, query_ids, pos_ids, weights, tau, upstream=None):
    """The reference's expressions (models/CGCL.py:95-127) in float64 on the device.  Returns the losses [nq], the gradient of
    sum_k up[k] loss[k] w.r.t. every distinct panel (in order of first appearance: table, then query panels) and pos / ttl
    of every block."""
    F = torch.nn.functional
    distinct, leaves = [], []
    for t in [table_panel] + list(query_panels):
        if not any(t is p for p in distinct):
            distinct.append(t)
            leaves.append(t.detach().double().requires_grad_(True))
    leaf = lambda t: leaves[[i for i, p in enumerate(distinct) if p is t][0]]  # noqa: E731
    Th = F.normalize(leaf(table_panel)[row0:row0 + N])
    losses, ratios = [], []
    for k, (qp, ids) in enumerate(zip(query_panels, query_ids)):
        q = F.normalize(leaf(qp)[ids])
        pos = torch.exp((q * Th[pos_ids]).sum(dim=1) / tau)
        ttl = torch.exp(q @ Th.T / tau).sum(dim=1)
        ratios.append((pos / ttl).detach())
        losses.append(weights[k] * -torch.log(pos / ttl + 10e-8).sum())
    up = [1.0] * len(losses) if upstream is None else upstream
    sum(u * l for u, l in zip(up, losses)).backward()
    return [l.item() for l in losses], [x.grad for x in leaves], ratios


def _close_grad(mine, ref, tol=1e-5):
    mine, ref = mine.double().cpu().numpy(), ref.cpu().numpy()
    np.testing.assert_allclose(mine, ref, rtol=0, atol=tol * np.abs(ref).max())


# --------------------------------------------------------------------------------------- 1. the operator
# (d, B, N, nq, row0, tau): every width path (32 .. 256 and the padded 48 / 100), B and N of one row, the 128-row tile
# remainders, a table that starts inside its panel, one and two query blocks
CASES = [(64, 96, 250, 2, 0, 0.1), (128, 96, 63, 1, 5, 0.2), (256, 1, 1, 1, 0, 1.0), (32, 96, 4097, 2, 3, 0.05),
         (48, 2048, 250, 1, 0, 0.1), (100, 96, 4097, 2, 7, 0.2), (64, 2048, 38048, 2, 100, 0.1), (256, 96, 4097, 1, 0, 0.1),
         (128, 1, 63, 2, 0, 1.0), (48, 1, 38048, 1, 0, 0.05), (100, 2048, 1, 1, 2, 0.2), (32, 2048, 63, 2, 0, 1.0),
         (64, 96, 128, 1, 0, 0.05), (64, 128, 129, 2, 1, 0.1),
         # the widths of 3, 5, 6 and 7 feature chunks (the score loop is unrolled up to 5 chunks and rolled above)
         (96, 96, 250, 2, 0, 0.1), (160, 96, 129, 1, 3, 0.2), (192, 1, 63, 1, 0, 1.0), (224, 96, 250, 2, 0, 0.1)]


@pytest.mark.parametrize("d,B,N,nq,row0,tau", CASES)
def test_op_matches_float64_torch(d, B, N, nq, row0, tau):
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(d * 7 + B * 3 + N + nq)
    n = row0 + N + 11
    table = torch.randn(n, d, device="cuda", generator=gen) * 0.3
    M = 500
    qps = [torch.randn(M, d, device="cuda", generator=gen) * (0.1 + k) for k in range(nq)]
    ids = [torch.randint(0, M, (B,), device="cuda", generator=gen) for _ in range(nq)]
    pos = torch.randint(0, N, (B,), device="cuda", generator=gen)
    if B >= 3:
        for i in ids:
            i[1], i[B - 1] = i[0], i[0]  # repeated query ids
        pos[2] = pos[0]
    weights = [0.7, 1.9][:nq]
    g_table = torch.zeros_like(table)
    g_q = [torch.zeros_like(q) for q in qps]
    loss = ops.table_nce_raw(table, row0, N, qps, ids, pos, weights, tau, g_table=g_table, g_queries=g_q)
    ref_loss, ref_g, _ = _ref64(table, row0, N, qps, ids, pos, weights, tau)
    print("losses", loss.cpu().numpy(), ref_loss)
    np.testing.assert_allclose(loss.cpu().numpy(), ref_loss, rtol=1e-5)
    for name, mine, ref in [("table", g_table, ref_g[0])] + [("query%d" % k, g_q[k], ref_g[1 + k]) for k in range(nq)]:
        err = (mine.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
        print(name, "max err / max|ref| = %.3g, max|ref| = %.3g" % (err, ref.abs().max().item()))
        if N == 1:
            # A table of one row: softmax - [j = pos] is 1 - 1, the true gradient is ZERO and the float64 reference holds
            # its own rounding residue (~1e-17), which cannot scale a bound.  The gradient is the difference of two terms of
            # size w / tau / ||x|| each; fp32 forms each to ~1e-7 of that, so that size takes the place of max|ref|.
            norms = torch.cat([table[row0:row0 + N].norm(dim=1)] + [q[i].norm(dim=1) for q, i in zip(qps, ids)])
            scale = max(weights) / tau / norms.min().item()
            assert ref.abs().max().item() < 1e-9 * scale
            assert mine.abs().max().item() <= 1e-5 * scale, (mine.abs().max().item(), scale)
        else:
            _close_grad(mine, ref)
    # rows outside [row0, row0 + N) of the table's gradient panel are not written
    assert not g_table[:row0].any() and not g_table[row0 + N:].any()
    # the loss-only call gives the same losses; a second call gives the same bits; gradients ADD into what the panels hold
    # (a row may receive two additions per call — the dense part and the positives' part — so twice the call is 2 x to
    # rounding, not to the bit)
    assert torch.equal(ops.table_nce_raw(table, row0, N, qps, ids, pos, weights, tau), loss)
    h_table, h_q = torch.zeros_like(table), [torch.zeros_like(q) for q in qps]
    loss2 = ops.table_nce_raw(table, row0, N, qps, ids, pos, weights, tau, g_table=h_table, g_queries=h_q)
    assert torch.equal(loss2, loss) and torch.equal(h_table, g_table)
    for a, b in zip(h_q, g_q):
        assert torch.equal(a, b)
    ops.table_nce_raw(table, row0, N, qps, ids, pos, weights, tau, g_table=h_table, g_queries=h_q)
    for a, b in zip([h_table] + h_q, [g_table] + g_q):
        torch.testing.assert_close(a, 2 * b, rtol=1e-6, atol=1e-6 * b.abs().max().item())


def test_upstream_scales_each_block():
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(5)
    d, B, N = 64, 300, 700
    table = torch.randn(N, d, device="cuda", generator=gen)
    qps = [torch.randn(400, d, device="cuda", generator=gen) for _ in range(2)]
    ids = [torch.randint(0, 400, (B,), device="cuda", generator=gen) for _ in range(2)]
    pos = torch.randint(0, N, (B,), device="cuda", generator=gen)
    up = torch.tensor([0.25, -3.0], device="cuda")
    g_table, g_q = torch.zeros_like(table), [torch.zeros_like(q) for q in qps]
    ops.table_nce_raw(table, 0, N, qps, ids, pos, [1.0, 0.5], 0.2, upstream=up, g_table=g_table, g_queries=g_q)
    _, ref_g, _ = _ref64(table, 0, N, qps, ids, pos, [1.0, 0.5], 0.2, upstream=[0.25, -3.0])
    for mine, ref in zip([g_table] + g_q, ref_g):
        _close_grad(mine, ref)


# --------------------------------------------------------------------------------------- 2. the guard regime
@pytest.mark.parametrize("N", [1000, 38048])
def test_guard_regime(N):
    """Positives that are the negated queries at tau = 0.1: pos / ttl is of the order of 1e-8, so the +1e-7 inside the log
    decides the loss and the factor r / (r + 1e-7) of the gradient."""
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(N)
    d, B, tau = 64, 256, 0.1
    table = torch.randn(N, d, device="cuda", generator=gen)
    pos = torch.randint(0, N, (B,), device="cuda", generator=gen)
    qp = -table.clone()
    g_table, g_q = torch.zeros_like(table), [torch.zeros_like(qp)]
    loss = ops.table_nce_raw(table, 0, N, [qp], [pos], pos, [1.0], tau, g_table=g_table, g_queries=g_q)
    ref_loss, ref_g, ratios = _ref64(table, 0, N, [qp], [pos], pos, [1.0], tau)
    print("median pos / ttl = %.3g, below the guard: %.3f" % (ratios[0].median().item(), (ratios[0] < 1e-7).float().mean().item()))
    assert (ratios[0] < 1e-7).float().mean().item() >= 0.5
    np.testing.assert_allclose(loss.cpu().numpy(), ref_loss, rtol=1e-5)
    _close_grad(g_table, ref_g[0])
    _close_grad(g_q[0], ref_g[1])


# --------------------------------------------------------------------------------------- 3. the autograd operator
@pytest.mark.parametrize("d", [48, 64])
def test_autograd_op_with_one_tensor_in_two_roles(d):
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(d)
    n, B, row0, N = 900, 200, 100, 650
    panel = (torch.randn(n, d, device="cuda", generator=gen) * 0.5).requires_grad_(True)
    other = (torch.randn(n, d, device="cuda", generator=gen) * 0.5).requires_grad_(True)
    ids0 = torch.randint(0, n, (B,), device="cuda", generator=gen)
    ids1 = torch.randint(0, n, (B,), device="cuda", generator=gen)
    ids0[3] = ids0[0]
    pos = torch.randint(0, N, (B,), device="cuda", generator=gen)
    # the panel is the table AND the first query panel: its gradients add
    l0, l1 = ops.table_nce_loss(panel, row0, N, [panel, other], [ids0, ids1], pos, [0.5, 2.0], 0.2)
    (3.0 * l0 - 0.5 * l1).backward()
    ref_loss, ref_g, _ = _ref64(panel, row0, N, [panel, other], [ids0, ids1], pos, [0.5, 2.0], 0.2, upstream=[3.0, -0.5])
    np.testing.assert_allclose([l0.item(), l1.item()], ref_loss, rtol=1e-5)
    assert len(ref_g) == 2
    _close_grad(panel.grad, ref_g[0])
    _close_grad(other.grad, ref_g[1])


# --------------------------------------------------------------------------------------- 4. reference goldens
@pytest.mark.parametrize("tag", ["def", "strong"])
def test_model_matches_reference_goldens(tag, tmp_path, golden_small, golden_cgcl):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.CGCL import CGCL

    g = golden_cgcl
    cfg = _cfg(**(STRONG if tag == "strong" else {}))
    data = _small_data(tmp_path, golden_small, cfg)
    tools.set_seed(2024)
    m = CGCL(cfg, data, torch.device("cuda")).to("cuda")
    b = torch.from_numpy(g["batch"]).cuda()
    users_emb, items_emb, layers = m.aggregate()
    assert users_emb.shape == (data.num_users, 64) and items_emb.shape == (data.num_items, 64) and len(layers) == 4
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 5
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-5)
    sum(ll).backward()
    for mine, ref in ((m.user_embedding.weight.grad, g[tag + "_grad_user"]), (m.item_embedding.weight.grad, g[tag + "_grad_item"])):
        print("grad max err / max|ref| = %.3g" % (np.abs(mine.cpu().numpy() - ref).max() / np.abs(ref).max()))
        np.testing.assert_allclose(mine.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
    m.eval()
    rating = m.get_rating_for_test(torch.from_numpy(g["rating_users"]).cuda())
    np.testing.assert_allclose(rating.cpu().numpy(), g[tag + "_rating"], rtol=1e-5, atol=1e-6)
    # the fused step, three batches, against the reference's own Adam trajectory
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    tools.set_seed(2024)
    m = CGCL(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 5), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        assert m.fused_train_step(*bt, loss[i], opt)
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    # (the trajectory criterion of tests/test_gpu_directau.py: Adam divides by sqrt(v), so where a gradient is of the order
    # of its own rounding error a last-place difference moves the element visibly)
    for mine, ref in ((m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])):
        mine = mine.detach().cpu().numpy()
        off = ~np.isclose(mine, ref, rtol=1e-4, atol=1e-6)
        print("trajectory: off %.3g, max %.3g" % (off.mean(), np.abs(mine - ref).max()))
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - ref).max() < 1e-4, np.abs(mine - ref).max()


def test_model_needs_two_layers(tmp_path, golden_small):
    from models.CGCL import CGCL

    cfg = _cfg(GCN_layer=1)
    data = _small_data(tmp_path, golden_small, cfg)
    with pytest.raises(ValueError, match="GCN_layer >= 2"):
        CGCL(cfg, data, torch.device("cuda"))


# --------------------------------------------------------------------------------------- 5. fused step == autograd step
@pytest.mark.parametrize("layers", [2, 3, 4])
def test_fused_step_equals_autograd_step(layers, tmp_path, golden_small):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.CGCL import CGCL

    cfg = _cfg(GCN_layer=layers, **STRONG)
    data = _small_data(tmp_path, golden_small, cfg)
    tri = torch.from_numpy(golden_small["sample1"][:3 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(3)]
    res = []
    for fused in (True, False):
        tools.set_seed(2024)
        model = CGCL(cfg, data, torch.device("cuda")).to("cuda")
        model.keep_fused_grad = True
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((3, 5), device="cuda")
        for i in range(3):
            if fused:
                assert model.fused_train_step(*bt[i], loss[i], opt)
            else:
                ll = model(*bt[i])
                loss[i] = torch.stack([x.detach() for x in ll])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
        st = opt.state[model.item_embedding.weight]
        assert st["step"] == 3
        res.append((loss.cpu().numpy(), model.user_embedding.weight.grad.cpu().numpy(), model._storage.cpu().numpy(),
                    opt.state[model.user_embedding.weight]["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()))
    (l_f, g_f, w_f, m_f, v_f), (l_a, g_a, w_a, m_a, v_a) = res
    np.testing.assert_allclose(l_f, l_a, rtol=2e-5)
    np.testing.assert_allclose(g_f, g_a, rtol=1e-3, atol=1e-5 * np.abs(g_a).max())
    np.testing.assert_allclose(w_f, w_a, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(m_f, m_a, rtol=1e-3, atol=1e-5 * np.abs(m_a).max())
    np.testing.assert_allclose(v_f, v_a, rtol=2e-3, atol=1e-6 * np.abs(v_a).max())


def test_fused_step_keeps_the_optimizer_state_as_the_source_of_truth(tmp_path, golden_small):
    """Fused steps and fused gradients + optimizer.step() interleave on one state, bit for bit."""
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.CGCL import CGCL

    cfg = _cfg(**STRONG)
    data = _small_data(tmp_path, golden_small, cfg)
    tri = torch.from_numpy(golden_small["sample1"][:4 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(4)]
    out = []
    for plan in ("TTTT", "FTFT"):
        tools.set_seed(2024)
        model = CGCL(cfg, data, torch.device("cuda")).to("cuda")
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((4, 5), device="cuda")
        for i, one_chain in enumerate(plan):
            if one_chain == "T":
                assert model.fused_train_step(*bt[i], loss[i], opt)
            else:
                model.fused_loss_and_grad(*bt[i], loss_out=loss[i])
                opt.step()
        st = opt.state[model.item_embedding.weight]
        assert st["step"] == 4
        out.append((model._storage.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), loss.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # an optimizer that is not ours is refused, nothing done
    model2 = CGCL(cfg, data, torch.device("cuda")).to("cuda")
    before = model2._storage.clone()
    assert not model2.fused_train_step(*bt[0], torch.zeros(5, device="cuda"), torch.optim.Adam(model2.parameters(), lr=0.001))
    assert torch.equal(before, model2._storage)


# --------------------------------------------------------------------------------------- 6. / 7. yelp2018 shape
@pytest.fixture(scope="module")
def yelp_data(tmp_path_factory):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    root = str(tmp_path_factory.mktemp("cgcl_yelp"))
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = _cfg(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0")
    return data_loader.Data(os.path.join(root, "yelp2018"), cfg), cfg


def test_fused_training_is_bit_reproducible_at_yelp_shape(yelp_data):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.CGCL import CGCL

    data, cfg = yelp_data
    np.random.seed(0)
    s = data.sample_data_to_train_all()
    tri = torch.from_numpy(s[:5 * 2048]).cuda()
    bt = [tuple(tri[i * 2048:(i + 1) * 2048, c].contiguous() for c in range(3)) for i in range(5)]
    out = []
    for run in range(2):
        tools.set_seed(2024)
        model = CGCL(cfg, data, torch.device("cuda")).to("cuda")
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((5, 5), device="cuda")
        for i in range(5):
            assert model.fused_train_step(*bt[i], loss[i], opt)
        st = opt.state[model.user_embedding.weight]
        out.append((model._storage.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), loss.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out[0][3]).all())


def test_no_batch_by_table_buffer():
    """At B = 2048, N = 38,048, d = 64, nq = 2 the workspace and the peak of the allocator over the call (outputs included)
    each stay below a quarter of ONE [B, N] fp32 matrix."""
    from idgrec_amd import native, ops

    B, N, d, nq = 2048, 38048, 64, 2
    quarter = B * N * 4 // 4
    assert 0 < native.lib.idg_table_nce_workspace_bytes(B, N, d, nq) < quarter
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.randn(N, d, device="cuda", generator=gen)
    qps = [torch.randn(N, d, device="cuda", generator=gen) for _ in range(nq)]
    ids = [torch.randint(0, N, (B,), device="cuda", generator=gen) for _ in range(nq)]
    pos = torch.randint(0, N, (B,), device="cuda", generator=gen)
    ops._tnce_ws_cache.clear()  # the call allocates its workspace: it counts
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    g_table, g_q = torch.zeros_like(table), [torch.zeros_like(q) for q in qps]
    outputs = g_table.numel() * 4 * (1 + nq)
    loss = ops.table_nce_raw(table, 0, N, qps, ids, pos, [1.0, 1.0], 0.1, g_table=g_table, g_queries=g_q)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak over the call: %.1f MB (gradient panels %.1f MB), quarter of [B, N]: %.1f MB" % (peak / 1e6, outputs / 1e6, quarter / 1e6))
    assert peak < quarter
    assert bool(torch.isfinite(loss).all())


# --------------------------------------------------------------------------------------- 8. end to end
def _numbers(text):
    return [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", text)]


@pytest.mark.parametrize("width,fused", [(64, True), (48, False)])
def test_trainer_end_to_end(width, fused, tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    S.make_dataset(str(tmp_path), "medium", n_test=8)
    cfg = _cfg(dataset="medium", dataset_path=str(tmp_path) + "/", sparsity_test="0", interval=1, top_K="[20]",
               test_batch_size=2048, training_epochs=2, batch_size=1024, embedding_size=width)
    data = data_loader.Data(str(tmp_path / "medium"), cfg)
    stream = io.StringIO()
    logger = logging.getLogger("cgcl_e2e_%d" % width)
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models.CGCL").Trainer(None, cfg, data, torch.device("cuda"), logger)
    calls = {"fused": 0, "forward": 0}
    fs, fw = tr.model.fused_train_step, tr.model.forward

    def count_fused(*a, **kw):
        calls["fused"] += 1
        return fs(*a, **kw)

    def count_forward(*a, **kw):
        calls["forward"] += 1
        return fw(*a, **kw)

    tr.model.fused_train_step, tr.model.forward = count_fused, count_forward
    tr.train()
    assert tr.model.fused_step_available() == fused
    assert (calls["fused"] > 0 and calls["forward"] == 0) if fused else (calls["fused"] == 0 and calls["forward"] > 0)
    lines = stream.getvalue().splitlines()
    loss_lines = [ln.split("training loss:")[1] for ln in lines if "training loss" in ln]
    recalls = [ln for ln in lines if "Test recall" in ln]
    assert len(loss_lines) == 2 and len(recalls) == 2
    for ln in loss_lines:
        assert re.fullmatch(r"\s*\S+ = \S+ \+ \S+ \+ \S+ \+ \S+ \+ \S+\s*", ln), ln  # five loss columns
        nums = _numbers(ln)
        assert len(nums) == 6 and np.isfinite(nums).all()
