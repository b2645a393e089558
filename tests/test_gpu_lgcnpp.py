"""LightGCN++ on the GPU: the two row-normalisation kernels against float64 across their dispatch (lane groups of 8 to 64,
one and two float4s per lane, the scalar path, zero rows, every allowed aliasing), ops.rows_normalize and
ops.propagate_normalized under autograd against the float64 chain of tests/lgcnpp_ref64.py, the model against the
reference's goldens in two settings, the fused training step against the autograd step, a width the fused step is not built
for, and training end to end."""
import functools
import importlib
import io
import itertools
import logging
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import lgcnpp_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
SETTINGS = {"def": dict(alpha=0.6, beta=-0.1, gamma=0.2), "skew": dict(alpha=0.2, beta=0.9, gamma=0.5)}
# (n, d, scale): a single row; fewer rows than one workgroup's; the padded widths 48 and 100, Xavier magnitude on the second;
# several values per lane, and the widest; a width that is not a multiple of 4
CASES = [(1, 64, 1.0), (3, 32, 1.0), (65, 48, 1.0), (130, 100, 0.02), (257, 256, 1.0), (70, 512, 1.0), (33, 7, 1.0)]


@pytest.fixture(scope="module")
def golden_pp():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "lgcnpp_small.npz")))


@functools.lru_cache(maxsize=None)
def _case(n, d, scale):
    """X with rows 0 and n - 1 exact zeros where n > 2, the other panels of the backward call, and the kernel's own forward
    result (computed once, left unchanged)."""
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(n * 131 + d)
    X = torch.randn(n, d, device="cuda", generator=gen) * scale
    zero = [0, n - 1] if n > 2 else []
    for r in zero:
        X[r] = 0
    T, G, A2 = (torch.randn(n, d, device="cuda", generator=gen) * s for s in (1.0, 0.5, scale))
    Y, norms = ops.rows_normalize_raw(X)
    return dict(X=X, T=T, G=G, A2=A2, Y=Y, norms=norms, zero=zero)


# --------------------------------------------------------------------------------------- 1. forward kernel
@pytest.mark.parametrize("n,d,scale", CASES)
def test_rows_normalize_matches_float64(n, d, scale):
    from idgrec_amd import ops

    c = _case(n, d, scale)
    X, Y, norms = c["X"], c["Y"], c["norms"]
    assert Y.shape == (n, d) and norms.shape == (n,) and Y.dtype == norms.dtype == torch.float32
    y64, n64 = ref.rownorm64(X)
    # bounds that hold for any summation order: d squares and d - 1 additions under a square root, one addition, one division
    en = (norms.double() - n64).abs()
    ey = (Y.double() - y64).abs()
    live = n64 > 0
    print("max |norms - n64| / bound = %.3g, max |Y - y64| / bound = %.3g"
          % (float((en[live] / ((d / 2 + 2) * U24 * n64[live])).max()) if bool(live.any()) else 0.0,
             float((ey[live] / ((d / 2 + 4) * U24 * y64[live].abs()).clamp_min(1e-300)).max()) if bool(live.any()) else 0.0))
    assert bool((en <= (d / 2 + 2) * U24 * n64).all())
    assert bool((ey <= (d / 2 + 4) * U24 * y64.abs()).all())
    for r in c["zero"]:
        assert float(norms[r]) == 0.0 and bool((Y[r] == 0).all())
    assert bool(torch.isfinite(Y).all())
    # the same bits again, into caller's buffers, and in place
    Y2, n2 = torch.full_like(X, 7.0), torch.full_like(norms, 7.0)
    ops.rows_normalize_raw(X, Y=Y2, norms=n2)
    assert torch.equal(Y2, Y) and torch.equal(n2, norms)
    Xi = X.clone()
    Yi, ni = ops.rows_normalize_raw(Xi, Y=Xi)
    assert Yi.data_ptr() == Xi.data_ptr() and torch.equal(Xi, Y) and torch.equal(ni, norms)


def test_rows_normalize_rejects_what_the_library_rejects_on_the_device():
    from idgrec_amd import ops

    X = torch.randn(16, 64, device="cuda")
    buf = torch.empty(17, 64, device="cuda")
    with pytest.raises(RuntimeError, match="overlaps X"):
        ops.rows_normalize_raw(X=buf[:16], Y=buf[1:])
    with pytest.raises(RuntimeError, match="norms overlaps"):
        ops.rows_normalize_raw(X, norms=X.view(-1)[:16])
    Y, norms = ops.rows_normalize_raw(X)
    with pytest.raises(RuntimeError, match="out overlaps Y or norms"):
        ops.rows_normalize_bwd_raw(X, Y, norms, out=Y)
    with pytest.raises(RuntimeError, match="without being it"):
        ops.rows_normalize_bwd_raw(buf[:16], Y, norms, out=buf[1:])
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.rows_normalize_raw(torch.empty(5, 7, device="cuda")[1:])


# --------------------------------------------------------------------------------------- 2. backward kernel
@pytest.mark.parametrize("n,d,scale", CASES)
def test_rows_normalize_bwd_matches_float64(n, d, scale):
    """out = a G + add2 + J(T) from the forward kernel's own Y and norms; the float64 reference is evaluated from those same
    Y, norms.  Tolerance: the float64 expression with every term replaced by its absolute value, times (d + 8) 2^-24 — the
    forward error bound of a d-term dot product plus the handful of remaining operations."""
    from idgrec_amd import ops

    c = _case(n, d, scale)
    T, Y, norms = c["T"], c["Y"], c["norms"]
    worst = 0.0
    for G, A2, a in itertools.product((None, c["G"]), (None, c["A2"]), (0.0, 0.2)):
        out = ops.rows_normalize_bwd_raw(T, Y, norms, G=G, a=a, add2=A2)
        want = ref.rownorm_bwd64(T, Y, norms, G=G, a=a, add2=A2)
        tol = (d + 8) * U24 * ref.rownorm_bwd_abs64(T, Y, norms, G=G, a=a, add2=A2)
        err = (out.double() - want).abs()
        worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
        assert bool(torch.isfinite(out).all())
        assert bool((err <= tol).all()), (G is not None, A2 is not None, a, float((err / tol.clamp_min(1e-300)).max()))
        for r in c["zero"]:  # a zero row with T != 0 returns t / eps (+ the other terms), within the same bound
            z = T[r].double() / ref.EPS + (a * G[r].double() if G is not None else 0) + (A2[r].double() if A2 is not None else 0)
            assert bool(((out[r].double() - z).abs() <= tol[r]).all()) and float(out[r].abs().max()) > 1e9
    print("largest observed error / tolerance = %.3g" % worst)


@pytest.mark.parametrize("n,d,scale", CASES)
def test_rows_normalize_bwd_allowed_aliasing_gives_the_same_bits(n, d, scale):
    from idgrec_amd import ops

    c = _case(n, d, scale)
    T, Y, norms, G, A2 = c["T"], c["Y"], c["norms"], c["G"], c["A2"]
    snap = {name: c[name].clone() for name in ("T", "Y", "norms", "G", "A2")}
    plain = ops.rows_normalize_bwd_raw(T, Y, norms, G=G, a=0.2, add2=A2)
    assert torch.equal(ops.rows_normalize_bwd_raw(T, Y, norms, G=G, a=0.2, add2=A2), plain)  # the same bits again
    t = T.clone()
    assert ops.rows_normalize_bwd_raw(t, Y, norms, G=G, a=0.2, add2=A2, out=t) is t and torch.equal(t, plain)
    g = G.clone()
    ops.rows_normalize_bwd_raw(T, Y, norms, G=g, a=0.2, add2=A2, out=g)
    assert torch.equal(g, plain)
    a2 = A2.clone()
    ops.rows_normalize_bwd_raw(T, Y, norms, G=G, a=0.2, add2=a2, out=a2)
    assert torch.equal(a2, plain)
    # inputs may alias one another: G == T, add2 == T, out == all three
    both = ops.rows_normalize_bwd_raw(T, Y, norms, G=T, a=0.2, add2=T)
    t = T.clone()
    ops.rows_normalize_bwd_raw(t, Y, norms, G=t, a=0.2, add2=t, out=t)
    assert torch.equal(t, both)
    for name, keep in snap.items():  # the shared case is left unchanged: only clones were written
        assert torch.equal(c[name], keep)


# --------------------------------------------------------------------------------------- 3. autograd
def _data(tmp_path, g, name, cfg):
    import utility.utility_data.data_loader as data_loader

    d = tmp_path / name
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset=name, dataset_path=str(tmp_path) + "/", sparsity_test="0")
    return data_loader.Data(str(d), cfg)


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN_pp.txt"), "LightGCN_pp")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


@pytest.mark.parametrize("n,d,scale", [(65, 48, 1.0), (33, 7, 1.0), (130, 64, 0.02)])
def test_rows_normalize_under_autograd(n, d, scale):
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(n + d)
    X = torch.randn(n, d, device="cuda", generator=gen) * scale
    X[n // 2] = 0
    W = torch.randn(n, d, device="cuda", generator=gen)
    x = X.clone().requires_grad_(True)
    y = ops.rows_normalize(x)
    (y * W).sum().backward()
    x64 = X.double().requires_grad_(True)
    y64 = x64 / (torch.norm(x64, dim=1) + ref.EPS)[:, None]
    (y64 * W.double()).sum().backward()
    assert bool(((y.detach().double() - y64.detach()).abs() <= (d / 2 + 4) * U24 * y64.detach().abs()).all())
    gr = x64.grad
    live = torch.ones(n, dtype=torch.bool, device="cuda")
    live[n // 2] = False
    np.testing.assert_allclose(x.grad[live].cpu().numpy(), gr[live].cpu().numpy(), rtol=1e-4,
                               atol=1e-5 * float(gr[live].abs().max()))
    np.testing.assert_allclose(x.grad[~live].cpu().numpy(), gr[~live].cpu().numpy(), rtol=1e-4)  # t / eps


@pytest.mark.parametrize("graph", ["tiny", "small"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("d", [64, 48])
def test_propagate_normalized_under_autograd(graph, K, d, tmp_path, golden_tiny, golden_small):
    import utility.utility_data.data_graph as data_graph
    import utility.utility_function.tools as tools
    from idgrec_amd import ops

    g = golden_tiny if graph == "tiny" else golden_small
    data = _data(tmp_path, g, graph, _cfg())
    s = SETTINGS["skew"]
    mat = data_graph.sparse_adjacency_matrix_asymmetric(data, s["alpha"], s["beta"])
    G = tools.convert_sp_mat_to_graph(mat, torch.device("cuda"), symmetric=False)
    assert not G.symmetric and G.T is not G and G.T.T is G
    n = mat.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(K * 100 + d)
    E0 = (torch.rand(n, d, device="cuda", generator=gen) - 0.5) * 0.2
    W = torch.randn(n, d, device="cuda", generator=gen)
    e = E0.clone().requires_grad_(True)
    final = ops.propagate_normalized(G, e, K, s["gamma"])
    (final * W).sum().backward()
    A64 = torch.from_numpy(mat.toarray().astype(np.float64)).cuda()
    e64 = E0.double().requires_grad_(True)
    f64 = ref.encoder64(A64, e64, K, s["gamma"])
    (f64 * W.double()).sum().backward()
    f64 = f64.detach()
    # a count of the roundings on the way to one output entry, taken relative to the largest entry: each layer is a
    # normalisation (d / 2 + 4 roundings) and a product of at most deg_max terms (deg_max roundings) plus the running sum
    # and the final combination (4 more), and a relative perturbation of a row at most doubles through the next
    # normalisation: 2 K (d / 2 + 8 + deg_max) 2^-24 max|ref|
    deg_max = int(np.diff(mat.indptr).max())
    atol = 2 * K * (d / 2 + 8 + deg_max) * U24 * float(f64.abs().max())
    err = float((final.detach().double() - f64).abs().max())
    print("output: max err %.3g, bound %.3g (deg_max %d)" % (err, atol, deg_max))
    assert err <= atol
    gr = e64.grad
    print("gradient: max err / max|ref| = %.3g" % (float((e.grad.double() - gr).abs().max()) / float(gr.abs().max())))
    np.testing.assert_allclose(e.grad.cpu().numpy(), gr.cpu().numpy(), rtol=1e-4, atol=1e-5 * float(gr.abs().max()))
    # the same bits again
    e2 = E0.clone().requires_grad_(True)
    f2 = ops.propagate_normalized(G, e2, K, s["gamma"])
    (f2 * W).sum().backward()
    assert torch.equal(f2, final) and torch.equal(e2.grad, e.grad)


# --------------------------------------------------------------------------------------- 4. reference goldens
@pytest.mark.parametrize("tag", ["def", "skew"])
def test_model_matches_reference_goldens(tag, tmp_path, golden_small, golden_pp):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.LightGCN_pp import LightGCN_pp

    g = golden_pp
    cfg = _cfg(**SETTINGS[tag])
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    m = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
    assert (m.alpha, m.beta, m.gamma) == tuple(g[tag + "_abg"]) and m.n_layers == 3
    assert np.array_equal(m.user_embedding.weight.detach().cpu().numpy(), g["init_user"])
    assert np.array_equal(m.item_embedding.weight.detach().cpu().numpy(), g["init_item"])
    assert not m.Graph.symmetric and m.Graph.T is not m.Graph
    b = torch.from_numpy(g["batch"]).cuda()
    users_emb, items_emb = m.aggregate()
    assert users_emb.shape == (data.num_users, 64) and items_emb.shape == (data.num_items, 64)
    m.zero_grad()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 2
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-5)
    sum(ll).backward()
    for mine, name in ((m.user_embedding.weight.grad, "user"), (m.item_embedding.weight.grad, "item")):
        want = g["%s_grad_%s" % (tag, name)]
        print("grad max err / max|ref| = %.3g" % (np.abs(mine.cpu().numpy() - want).max() / np.abs(want).max()))
        np.testing.assert_allclose(mine.cpu().numpy(), want, rtol=1e-4, atol=1e-5 * np.abs(want).max())
    # the fused gradient against the same goldens
    loss = m.fused_loss_and_grad(b[:, 0], b[:, 1], b[:, 2])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_loss"], rtol=1e-5)
    for mine, name in ((m.user_embedding.weight.grad, "user"), (m.item_embedding.weight.grad, "item")):
        want = g["%s_grad_%s" % (tag, name)]
        np.testing.assert_allclose(mine.cpu().numpy(), want, rtol=1e-4, atol=1e-5 * np.abs(want).max())
    m.eval()
    users = torch.from_numpy(g["rating_users"]).cuda()
    rating = m.get_rating_for_test(users)
    np.testing.assert_allclose(rating.cpu().numpy(), g[tag + "_rating"], rtol=1e-5, atol=1e-6)
    # the fused top-K ranks by this encoder as well: its first ranks are the best unseen items of the dense ratings
    top = m.topk_for_test(users, 5)
    masked = rating.clone()
    ip, ix = data.train_csr_on(rating.device)
    for i, u in enumerate(users.tolist()):
        masked[i, ix[int(ip[u]):int(ip[u + 1])].long()] = -1
    np.testing.assert_allclose(masked.gather(1, top.long()).sort(dim=1, descending=True).values.cpu().numpy(),
                               torch.topk(masked, 5).values.cpu().numpy(), rtol=1e-5)
    # three fused steps against the reference's own Adam trajectory
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    tools.set_seed(2024)
    m = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 2), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    # (the trajectory criterion of tests/test_gpu_cgcl.py: Adam divides by sqrt(v), so where a gradient is of the order of
    # its own rounding error a last-place difference moves the element visibly)
    for mine, want in ((m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])):
        mine = mine.detach().cpu().numpy()
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("trajectory: off %.3g, max %.3g" % (off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - want).max() < 1e-4, np.abs(mine - want).max()


# --------------------------------------------------------------------------------------- 5. fused step == autograd step
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_fused_step_equals_autograd_step(layers, tmp_path, golden_small):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.LightGCN_pp import LightGCN_pp

    cfg = _cfg(GCN_layer=layers, **SETTINGS["skew"])
    data = _data(tmp_path, golden_small, "small", cfg)
    tri = torch.from_numpy(golden_small["sample1"][:3 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(3)]
    res = []
    for fused in (True, False):
        tools.set_seed(2024)
        model = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
        model.keep_fused_grad = True
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((3, 2), device="cuda")
        for i in range(3):
            if fused:
                assert model.fused_train_step(*bt[i], loss[i], opt)
            else:
                ll = model(*bt[i])
                assert len(ll) == 2
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
    from models.LightGCN_pp import LightGCN_pp

    cfg = _cfg(**SETTINGS["skew"])
    data = _data(tmp_path, golden_small, "small", cfg)
    tri = torch.from_numpy(golden_small["sample1"][:4 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(4)]
    out = []
    for plan in ("TTTT", "FTFT"):
        tools.set_seed(2024)
        model = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((4, 2), device="cuda")
        for i, one_chain in enumerate(plan):
            if one_chain == "T":
                assert model.fused_train_step(*bt[i], loss[i], opt)
                assert model.user_embedding.weight.grad is None
            else:
                model.fused_loss_and_grad(*bt[i], loss_out=loss[i])
                opt.step()
        st = opt.state[model.item_embedding.weight]
        assert st["step"] == 4 and opt.state[model.user_embedding.weight]["step"] == 4
        out.append((model._storage.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), loss.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # the step's buffers are allocated once per storage
    buf = model._buf
    model.fused_loss_and_grad(*bt[0])
    assert model._buf is buf
    # an optimizer that is not ours is refused, nothing done
    model2 = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
    before = model2._storage.clone()
    assert not model2.fused_train_step(*bt[0], torch.zeros(2, device="cuda"), torch.optim.Adam(model2.parameters(), lr=0.001))
    assert torch.equal(before, model2._storage)


# --------------------------------------------------------------------------------------- 6. a width outside the fused step's
def test_width_48_trains_and_matches_the_float64_gradient(tmp_path, golden_small):
    import utility.utility_function.losses as losses
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.LightGCN_pp import LightGCN_pp

    cfg = _cfg(embedding_size=48, **SETTINGS["skew"])
    data = _data(tmp_path, golden_small, "small", cfg)
    U, I = data.num_users, data.num_items
    tools.set_seed(2024)
    m = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
    m.keep_fused_grad = True
    opt = ops.Adam(m.parameters(), lr=0.001)
    tri = torch.from_numpy(golden_small["sample1"][:256]).cuda()
    users, pos, neg = (tri[:, c].contiguous() for c in range(3))
    # the float64 chain on the initial tables
    import utility.utility_data.data_graph as data_graph

    mat = data_graph.sparse_adjacency_matrix_asymmetric(data, m.alpha, m.beta)
    A64 = torch.from_numpy(mat.toarray().astype(np.float64)).cuda()
    e64 = m._storage.detach().double().clone().requires_grad_(True)
    fu, fi = torch.split(ref.encoder64(A64, e64, m.n_layers, m.gamma), [U, I])
    eu, ei = torch.split(e64, [U, I])
    l64 = [losses.get_bpr_loss(fu[users], fi[pos], fi[neg]), m.reg_lambda * losses.get_reg_loss(eu[users], ei[pos], ei[neg])]
    sum(l64).backward()
    before = m._storage.clone()
    loss = torch.zeros(2, device="cuda")
    if m.fused_step_available():
        assert m.fused_train_step(users, pos, neg, loss, opt)
    else:
        ll = m(users, pos, neg)
        loss = torch.stack([x.detach() for x in ll])
        opt.zero_grad()
        sum(ll).backward()
        opt.step()
    np.testing.assert_allclose(loss.cpu().numpy(), [x.item() for x in l64], rtol=1e-5)
    mine = torch.cat([m.user_embedding.weight.grad, m.item_embedding.weight.grad]).cpu().numpy()
    want = e64.grad.cpu().numpy()
    print("grad max err / max|ref| = %.3g" % (np.abs(mine - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(mine, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())
    assert opt.state[m.user_embedding.weight]["step"] == 1 and not torch.equal(before, m._storage)
    # the step moved every row that has a gradient by about the step size against its sign
    moved = (m._storage - before).cpu().numpy()
    big = np.abs(want) > 1e-3 * np.abs(want).max()
    assert (np.sign(moved[big]) == -np.sign(want[big])).all()


# --------------------------------------------------------------------------------------- 7. end to end
def test_trainer_end_to_end(tmp_path, golden_small):
    import utility.utility_function.tools as tools

    cfg = _cfg(training_epochs=2, interval=1, top_K="[20]", test_batch_size=2048, batch_size=128, learn_rate=0.01)
    data = _data(tmp_path, golden_small, "small", cfg)
    stream = io.StringIO()
    logger = logging.getLogger("lgcnpp_e2e")
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models.LightGCN_pp").Trainer(None, cfg, data, torch.device("cuda"), logger)
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
    assert calls["fused"] > 0 and calls["forward"] == 0
    lines = stream.getvalue().splitlines()
    loss_lines = [ln.split("training loss:")[1] for ln in lines if "training loss" in ln]
    recalls = [float(re.search(r"Test recall: \[([^\],]+)", ln).group(1)) for ln in lines if "Test recall" in ln]
    assert len(loss_lines) == 2 and len(recalls) == 2
    totals = []
    for ln in loss_lines:
        terms = [float(x) for x in ln.split("=")[1].split("+")]
        assert len(terms) == 2 and np.isfinite(terms).all()
        totals.append(float(ln.split("=")[0]))
    print("loss per epoch", totals, "recall@20 per epoch", recalls)
    assert np.isfinite(totals).all() and totals[1] < totals[0]
    assert all(0.0 <= r <= 1.0 for r in recalls) and recalls[-1] > 0.0
