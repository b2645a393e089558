"""NCL on the GPU: the k-means kernels against float64 (assignment with its rounding bound, ties, strided panels; update with
empty clusters; whole runs on planted and Gaussian data, determinism), the model against the reference's goldens in two
settings before and after the warm-up, the fused training step against the autograd step, the memory condition (no [N, K]
buffer), and training end to end with the E-step in the loop."""
import functools
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
STRONG = dict(ssl_lambda=0.1, proto_lambda=1e-3, alpha=0.6)
# (N, K, d, scale): one row and one centroid; fewer than a tile of either; a tile plus one row; the padded widths 48 and
# 100 and the widest; K split over workgroups (few row tiles) with a partial last tile; rows of the magnitude of a
# Xavier-initialised table
CASES = [(1, 1, 64, 1.0), (127, 2, 32, 1.0), (129, 127, 256, 1.0), (500, 16, 64, 1.0), (4097, 129, 48, 1.0),
         (4097, 2000, 64, 1.0), (4097, 2000, 100, 1.0), (900, 40, 64, 0.02),
         # the widths of 3, 5, 6 and 7 feature chunks (the score loop is unrolled up to 5 chunks and rolled above)
         (129, 127, 96, 1.0), (129, 127, 160, 1.0), (500, 16, 192, 1.0), (129, 127, 224, 1.0)]


@pytest.fixture(scope="module")
def golden_ncl():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ncl_small.npz")))


def _dist64(X, C):
    """float64 squared distances [N, K] (the expanded form, evaluated in float64: its rounding is ~1e-16 of the norms)."""
    X, C = X.double(), C.double()
    return ((X * X).sum(1)[:, None] - 2.0 * X @ C.T + (C * C).sum(1)[None, :]).clamp_min(0)


def _means64(X, assign, C_before):
    """(float64 means of the rows per cluster — the centroid it had for a cluster without rows —, counts)."""
    K = C_before.shape[0]
    cnt = torch.bincount(assign.long(), minlength=K)
    s = torch.zeros(K, X.shape[1], dtype=torch.float64, device=X.device).index_add_(0, assign.long(), X.double())
    return torch.where(cnt[:, None] > 0, s / cnt.clamp_min(1)[:, None], C_before.double()), cnt


def _tol(X, C):
    """tol_i = 4 d 2^-24 (||x_i|| + max_j ||c_j||)^2: the rounding bound of the fp32 form ||c||^2 - 2 <x, c>."""
    d = X.shape[1]
    return 4.0 * d * 2.0 ** -24 * (X.double().norm(dim=1) + C.double().norm(dim=1).max()) ** 2


@functools.lru_cache(maxsize=None)
def _case(N, K, d, scale):
    """Gaussian X, C = K distinct rows of X after one float64 Lloyd update, and the float64 reference of the pair."""
    gen = torch.Generator(device="cuda").manual_seed(N * 31 + K * 7 + d)
    X = torch.randn(N, d, device="cuda", generator=gen) * scale
    first = torch.randperm(N, generator=torch.Generator().manual_seed(N + K))[:K].cuda()
    C0 = X[first].clone()
    C = _means64(X, _dist64(X, C0).argmin(dim=1), C0)[0].float().contiguous()
    D = _dist64(X, C)
    best2 = torch.topk(D, min(2, K), dim=1, largest=False).values
    gap = best2[:, 1] - best2[:, 0] if K > 1 else torch.full((N,), float("inf"), device="cuda", dtype=torch.float64)
    return dict(X=X, C=C, D=D, arg=D.argmin(dim=1), dmin=best2[:, 0], gap=gap, tol=_tol(X, C))


def _check_nearest(X, C, assign, dist2=None, ref=None):
    """The assignment is nearest-centroid up to the rounding bound, and exact wherever float64 separates best from second
    best by at least the bound."""
    N = X.shape[0]
    if ref is None:
        D = _dist64(X, C)
        b2 = torch.topk(D, min(2, C.shape[0]), dim=1, largest=False).values
        ref = dict(D=D, arg=D.argmin(dim=1), dmin=b2[:, 0], tol=_tol(X, C),
                   gap=b2[:, 1] - b2[:, 0] if C.shape[0] > 1 else torch.full((N,), float("inf"), device=X.device,
                                                                             dtype=torch.float64))
    a = assign.long()
    assert assign.dtype == torch.int32 and int(a.min()) >= 0 and int(a.max()) < C.shape[0]
    clear = ref["gap"] >= ref["tol"]
    print("rows with a float64 gap below the bound: %d of %d" % (int((~clear).sum()), N))
    assert int((~clear).sum()) <= 0.01 * N  # a property of the float64 reference alone
    mine = ref["D"].gather(1, a[:, None])[:, 0]
    excess = mine - ref["dmin"]
    print("max (D[i, assign_i] - min_j D[i, j]) / tol_i = %.3g" % float((excess / ref["tol"]).max()))
    assert bool((excess <= ref["tol"]).all())
    assert torch.equal(a[clear], ref["arg"][clear])
    if dist2 is not None:
        err = (dist2.double() - mine).abs()
        print("max |dist2 - D[i, assign_i]| / tol_i = %.3g" % float((err / ref["tol"]).max()))
        assert bool((dist2 >= 0).all()) and bool((err <= ref["tol"]).all())


# --------------------------------------------------------------------------------------- 1. assign
@pytest.mark.parametrize("N,K,d,scale", CASES)
def test_assign_matches_float64(N, K, d, scale):
    from idgrec_amd import ops

    c = _case(N, K, d, scale)
    X, C = c["X"], c["C"]
    dist2 = torch.empty(N, device="cuda")
    assign = ops.kmeans_assign_raw(X, C, dist2=dist2)
    _check_nearest(X, C, assign, dist2, ref=c)
    # the same bits again, and without dist2
    assert torch.equal(ops.kmeans_assign_raw(X, C), assign)
    # a panel with ldx > d gives the same answers as its packed copy
    wide = torch.randn(N, d + 7, device="cuda")
    wide[:, 3:3 + d] = X
    d2w = torch.empty(N, device="cuda")
    aw = ops.kmeans_assign_raw(wide[:, 3:3 + d], C, dist2=d2w)
    assert torch.equal(aw, assign) and torch.equal(d2w, dist2)


@pytest.mark.parametrize("N,K,d,scale", [c for c in CASES if c[1] >= 10])
def test_assign_sends_exact_ties_to_the_lowest_index(N, K, d, scale):
    from idgrec_amd import ops

    c = _case(N, K, d, scale)
    C = c["C"].clone()
    C[5] = c["X"][0]  # row 0 is at distance 0 of the tied centroid: the tie is met
    C[3], C[9] = C[5], C[5]
    far = K - 1 if K > 130 else None  # the same centroid again in another tile (and another chunk where K is split)
    if far is not None:
        C[far] = C[5]
    assign = ops.kmeans_assign_raw(c["X"], C)
    hist = torch.bincount(assign.long(), minlength=K)
    print("rows of the tied centroid: %d, row 0 -> %d" % (int(hist[3]), int(assign[0])))
    assert int(assign[0]) <= 3 and int(hist[5]) == 0 and int(hist[9]) == 0
    assert far is None or int(hist[far]) == 0


# --------------------------------------------------------------------------------------- 2. update
@pytest.mark.parametrize("N,K,d,scale", CASES)
def test_update_matches_float64_means(N, K, d, scale):
    from idgrec_amd import ops

    c = _case(N, K, d, scale)
    X = c["X"]
    assign = c["arg"].to(torch.int32).contiguous()
    ref, cnt = _means64(X, assign, c["C"])
    C = c["C"].clone()
    counts = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    assert ops.kmeans_update_raw(X, assign, C, counts=counts) is C
    err = (C.double() - ref).abs().max().item()
    print("max err %.3g, max|ref| %.3g" % (err, ref.abs().max().item()))
    assert err <= 1e-5 * ref.abs().max().item()
    assert torch.equal(counts.long(), cnt)
    # a cluster without rows keeps its centroid bit for bit: up to two clusters are emptied into a third
    empty = [j for j in (0, K - 1) if K >= 3] or ([1] if K == 2 else [])
    if empty:
        keep = 1 if K >= 3 else 0
        a2 = assign.clone()
        for j in empty:
            a2[a2 == j] = keep
        ref2, cnt2 = _means64(X, a2, c["C"])
        C2 = c["C"].clone()
        ops.kmeans_update_raw(X, a2, C2, counts=counts)
        for j in empty:
            assert torch.equal(C2[j], c["C"][j]) and int(counts[j]) == 0
        assert torch.equal(counts.long(), cnt2)
        assert (C2.double() - ref2).abs().max().item() <= 1e-5 * ref2.abs().max().item()
    # a strided panel
    wide = torch.randn(N, d + 5, device="cuda")
    wide[:, :d] = X
    C3 = c["C"].clone()
    ops.kmeans_update_raw(wide[:, :d], assign, C3)
    assert torch.equal(C3, C)


# --------------------------------------------------------------------------------------- 3. whole runs
@pytest.mark.parametrize("N", [800, 4097])
def test_planted_clusters_are_recovered(N):
    from idgrec_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(N)
    d, nb = 64, 8
    centres = torch.nn.functional.normalize(torch.randn(nb, d, device="cuda", generator=gen)) * 5.0
    blob = torch.arange(N, device="cuda") % nb
    X = centres[blob] + 0.05 * torch.randn(N, d, device="cuda", generator=gen)
    C = X[:nb].clone()  # row j belongs to blob j
    inertia = torch.empty(6, device="cuda")
    C_out, assign = ops.kmeans_raw(X, C, 5, inertia=inertia)
    assert C_out is C and torch.equal(assign.long(), blob)
    ref = _means64(X, blob, C)[0]
    print("max centroid error %.3g" % (C.double() - ref).abs().max().item())
    assert (C.double() - ref).abs().max().item() <= 1e-5
    np.testing.assert_allclose(inertia[-1].item(), _dist64(X, C).gather(1, blob[:, None]).sum().item(), rtol=1e-4)


def test_lloyd_iterations_on_gaussian_data():
    from idgrec_amd import ops

    N, K, d = 4097, 129, 64
    X = torch.randn(N, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    C, assign, inertia = ops.kmeans(X, K, niter=10, seed=1234)
    assert C.shape == (K, d) and assign.shape == (N,) and assign.dtype == torch.int32 and inertia.shape == (11,)
    it = inertia.cpu().numpy()
    print("inertia", it)
    assert np.isfinite(it).all() and (it[1:] <= it[:-1] * (1 + 1e-5)).all() and it[-1] < 0.95 * it[0]
    # the final assignment is nearest-centroid for the final centroids
    _check_nearest(X, C, assign)
    np.testing.assert_allclose(it[-1], _dist64(X, C).gather(1, assign.long()[:, None]).sum().item(), rtol=1e-4)
    # the documented initialisation, and every centroid the mean of its rows from the last-but-one assignment: nine
    # iterations from the same start end with that assignment
    first = torch.randperm(N, generator=torch.Generator().manual_seed(1234))[:K].cuda()
    assert len(set(first.tolist())) == K
    C9, a9 = ops.kmeans_raw(X, X[first].clone(), 9)
    ref, cnt = _means64(X, a9, C9)
    assert (C.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    # niter = 0: the initial centroids untouched and one assignment
    C0, a0, i0 = ops.kmeans(X, K, niter=0, seed=1234)
    assert torch.equal(C0, X[first]) and i0.shape == (1,) and torch.equal(a0, ops.kmeans_assign_raw(X, X[first].clone()))
    np.testing.assert_allclose(i0.item(), it[0], rtol=1e-6)
    with pytest.raises(ValueError, match="clusters for N"):
        ops.kmeans(X[:100], 101)


@pytest.mark.parametrize("N,K,d,niter", [(4097, 129, 48, 10), (31668, 2000, 64, 25)])
def test_two_runs_give_identical_bits(N, K, d, niter):
    from idgrec_amd import ops

    X = torch.randn(N, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N)) * 0.02
    a = ops.kmeans(X, K, niter=niter)
    b = ops.kmeans(X, K, niter=niter)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(a[2]).all()) and int(a[1].min()) >= 0 and int(a[1].max()) < K


# --------------------------------------------------------------------------------------- 4. reference goldens
def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "NCL.txt"), "NCL")
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


def _load_clusters(m, g):
    m.user_centroids, m.user_2cluster = torch.from_numpy(g["user_centroids"]).cuda(), torch.from_numpy(g["user_2cluster"]).cuda()
    m.item_centroids, m.item_2cluster = torch.from_numpy(g["item_centroids"]).cuda(), torch.from_numpy(g["item_2cluster"]).cuda()


@pytest.mark.parametrize("tag", ["def", "strong"])
def test_model_matches_reference_goldens(tag, tmp_path, golden_small, golden_ncl):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.NCL import NCL

    g = golden_ncl
    cfg = _cfg(k=16, **(STRONG if tag == "strong" else {}))
    data = _small_data(tmp_path, golden_small, cfg)
    tools.set_seed(2024)
    m = NCL(cfg, data, torch.device("cuda")).to("cuda")
    _load_clusters(m, g)
    b = torch.from_numpy(g["batch"]).cuda()
    users_emb, items_emb, layers = m.aggregate()
    assert users_emb.shape == (data.num_users, 64) and items_emb.shape == (data.num_items, 64) and len(layers) == 4
    for epoch, n_terms in ((0, 3), (20, 4)):
        m.zero_grad()
        ll = m(b[:, 0], b[:, 1], b[:, 2], epoch)
        assert len(ll) == n_terms
        ref = g["%s_loss%d" % (tag, epoch)]
        print("epoch", epoch, "losses", [x.item() for x in ll], ref)
        np.testing.assert_allclose([x.item() for x in ll], ref, rtol=1e-5)
        sum(ll).backward()
        for mine, name in ((m.user_embedding.weight.grad, "user"), (m.item_embedding.weight.grad, "item")):
            ref = g["%s_grad_%s%d" % (tag, name, epoch)]
            print("grad max err / max|ref| = %.3g" % (np.abs(mine.cpu().numpy() - ref).max() / np.abs(ref).max()))
            np.testing.assert_allclose(mine.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
    # the stored epoch stands in for the argument
    m.epoch = 20
    assert len(m(b[:, 0], b[:, 1], b[:, 2])) == 4
    m.epoch = 0
    assert len(m(b[:, 0], b[:, 1], b[:, 2])) == 3
    m.eval()
    rating = m.get_rating_for_test(torch.from_numpy(g["rating_users"]).cuda())
    np.testing.assert_allclose(rating.cpu().numpy(), g[tag + "_rating"], rtol=1e-5, atol=1e-6)
    # the fused step, three batches at epoch 20 with the clusters held fixed, against the reference's own Adam trajectory
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    tools.set_seed(2024)
    m = NCL(cfg, data, torch.device("cuda")).to("cuda")
    _load_clusters(m, g)
    m.epoch = 20
    assert m.fused_step_available()
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 4), device="cuda")
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        assert m.fused_train_step(*bt, loss[i], opt)
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    # (the trajectory criterion of tests/test_gpu_cgcl.py: Adam divides by sqrt(v), so where a gradient is of the order of
    # its own rounding error a last-place difference moves the element visibly)
    for mine, ref in ((m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])):
        mine = mine.detach().cpu().numpy()
        off = ~np.isclose(mine, ref, rtol=1e-4, atol=1e-6)
        print("trajectory: off %.3g, max %.3g" % (off.mean(), np.abs(mine - ref).max()))
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - ref).max() < 1e-4, np.abs(mine - ref).max()


def test_model_refuses_settings_it_cannot_run(tmp_path, golden_small):
    from models.NCL import NCL

    cfg = _cfg(k=16, GCN_layer=1, cl_layer=1)
    data = _small_data(tmp_path, golden_small, cfg)
    with pytest.raises(ValueError, match="GCN_layer >= 2 \\* cl_layer"):
        NCL(cfg, data, torch.device("cuda"))
    with pytest.raises(ValueError, match="k = 251 clusters"):
        NCL(_cfg(k=251, dataset="small", dataset_path=str(tmp_path) + "/"), data, torch.device("cuda"))
    m = NCL(_cfg(k=250, dataset="small", dataset_path=str(tmp_path) + "/"), data, torch.device("cuda")).to("cuda")
    with pytest.raises(RuntimeError, match="needs clusters"):
        m(torch.zeros(4, dtype=torch.long, device="cuda"), torch.zeros(4, dtype=torch.long, device="cuda"),
          torch.ones(4, dtype=torch.long, device="cuda"), 20)
    m.E_step()  # k = the smaller table: every item its own cluster
    assert m.item_centroids.shape == (250, 64) and m.user_2cluster.shape == (300,) and m.user_2cluster.dtype == torch.int64
    assert len(set(m.item_2cluster.tolist())) == 250
    P = m._proto_panel()
    assert torch.equal(P[:300], m.user_centroids[m.user_2cluster]) and torch.equal(P[300:], m.item_centroids[m.item_2cluster])


# --------------------------------------------------------------------------------------- 5. fused step == autograd step
@pytest.mark.parametrize("layers,epoch", [(2, 0), (2, 20), (3, 0), (3, 20)])
def test_fused_step_equals_autograd_step(layers, epoch, tmp_path, golden_small, golden_ncl):
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.NCL import NCL

    cfg = _cfg(k=16, GCN_layer=layers, **STRONG)
    data = _small_data(tmp_path, golden_small, cfg)
    tri = torch.from_numpy(golden_small["sample1"][:3 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(3)]
    res = []
    for fused in (True, False):
        tools.set_seed(2024)
        model = NCL(cfg, data, torch.device("cuda")).to("cuda")
        _load_clusters(model, golden_ncl)
        model.epoch = epoch
        model.keep_fused_grad = True
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((3, 4), device="cuda")
        for i in range(3):
            if fused:
                assert model.fused_train_step(*bt[i], loss[i], opt)
            else:
                ll = model(*bt[i])
                assert len(ll) == (3 if epoch == 0 else 4)
                loss[i, :len(ll)] = torch.stack([x.detach() for x in ll])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
        st = opt.state[model.item_embedding.weight]
        assert st["step"] == 3
        res.append((loss.cpu().numpy(), model.user_embedding.weight.grad.cpu().numpy(), model._storage.cpu().numpy(),
                    opt.state[model.user_embedding.weight]["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()))
    (l_f, g_f, w_f, m_f, v_f), (l_a, g_a, w_a, m_a, v_a) = res
    assert (l_f[:, 3] == 0).all() if epoch == 0 else (l_f[:, 3] > 0).all()
    np.testing.assert_allclose(l_f, l_a, rtol=2e-5)
    np.testing.assert_allclose(g_f, g_a, rtol=1e-3, atol=1e-5 * np.abs(g_a).max())
    np.testing.assert_allclose(w_f, w_a, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(m_f, m_a, rtol=1e-3, atol=1e-5 * np.abs(m_a).max())
    np.testing.assert_allclose(v_f, v_a, rtol=2e-3, atol=1e-6 * np.abs(v_a).max())


def test_fused_step_keeps_the_optimizer_state_as_the_source_of_truth(tmp_path, golden_small, golden_ncl):
    """Fused steps and fused gradients + optimizer.step() interleave on one state, bit for bit."""
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.NCL import NCL

    cfg = _cfg(k=16, **STRONG)
    data = _small_data(tmp_path, golden_small, cfg)
    tri = torch.from_numpy(golden_small["sample1"][:4 * 256]).cuda()
    bt = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(4)]
    out = []
    for plan in ("TTTT", "FTFT"):
        tools.set_seed(2024)
        model = NCL(cfg, data, torch.device("cuda")).to("cuda")
        _load_clusters(model, golden_ncl)
        model.epoch = 20
        opt = ops.Adam(model.parameters(), lr=0.001)
        loss = torch.zeros((4, 4), device="cuda")
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
    model2 = NCL(cfg, data, torch.device("cuda")).to("cuda")
    before = model2._storage.clone()
    assert not model2.fused_train_step(*bt[0], torch.zeros(4, device="cuda"), torch.optim.Adam(model2.parameters(), lr=0.001))
    assert torch.equal(before, model2._storage)


# --------------------------------------------------------------------------------------- yelp2018 shape
def test_fused_training_with_the_e_step_is_bit_reproducible_at_yelp_shape(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools
    from idgrec_amd import ops
    from models.NCL import NCL

    S.make_dataset(str(tmp_path), "yelp2018", n_test=1)
    cfg = _cfg(dataset="yelp2018", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "yelp2018"), cfg)
    np.random.seed(0)
    s = data.sample_data_to_train_all()
    tri = torch.from_numpy(s[:3 * 2048]).cuda()
    bt = [tuple(tri[i * 2048:(i + 1) * 2048, c].contiguous() for c in range(3)) for i in range(3)]
    out = []
    for run in range(2):
        tools.set_seed(2024)
        model = NCL(cfg, data, torch.device("cuda")).to("cuda")
        opt = ops.Adam(model.parameters(), lr=0.001)
        model.begin_epoch(20)  # the E-step: k = 2000, 25 iterations, both tables
        loss = torch.zeros((3, 4), device="cuda")
        for i in range(3):
            assert model.fused_train_step(*bt[i], loss[i], opt)
        st = opt.state[model.user_embedding.weight]
        out.append((model._storage.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), loss.clone(),
                    model.user_centroids.clone(), model.user_2cluster.clone(), model.item_centroids.clone(),
                    model.item_2cluster.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out[0][3]).all()) and bool((out[0][3][:, 3] > 0).all())
    assert out[0][4].shape == (2000, 64) and out[0][7].shape == (data.num_items,)


# --------------------------------------------------------------------------------------- 6. memory
def test_no_rows_by_centroids_buffer():
    """At N = 38,048, K = 2000, d = 64 the workspace, and the peak of the allocator over a call (outputs included), stay
    below ONE [N, K] fp32 matrix."""
    from idgrec_amd import native, ops

    N, K, d = 38048, 2000, 64
    full = N * K * 4
    ws_bytes = native.lib.idg_kmeans_workspace_bytes(N, K, d)
    print("workspace %.1f MB, [N, K] fp32 %.1f MB" % (ws_bytes / 1e6, full / 1e6))
    assert 0 < ws_bytes < full
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(N, d, device="cuda", generator=gen)
    C = X[:K].clone()
    first = ops.kmeans_assign_raw(X, C, dist2=torch.empty(N, device="cuda"))  # the warm-up call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dist2 = torch.empty(N, device="cuda")
    assign = ops.kmeans_assign_raw(X, C, dist2=dist2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak over the call: %.3f MB" % (peak / 1e6))
    assert peak < full
    # with the workspace counted as well
    ops._kmeans_ws_cache.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    again = ops.kmeans_assign_raw(X, C)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < full
    assert torch.equal(again, assign) and torch.equal(first, assign) and bool((assign[:K].long() == torch.arange(K, device="cuda")).all())


# --------------------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("width,fused", [(64, True), (48, False)])
def test_trainer_end_to_end(width, fused, tmp_path, golden_small):
    import utility.utility_function.tools as tools

    # the file's loss weights, where BPR drives the training (with the strong weights of the golden tests the contrastive
    # terms do, and ranking quality is not what they optimise); 24 steps an epoch at a step size that moves the tables
    cfg = _cfg(k=16, proto_warmup=1, training_epochs=3, interval=1, top_K="[20]", test_batch_size=2048, batch_size=128,
               embedding_size=width, learn_rate=0.01)
    data = _small_data(tmp_path, golden_small, cfg)
    stream = io.StringIO()
    logger = logging.getLogger("ncl_e2e_%d" % width)
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models.NCL").Trainer(None, cfg, data, torch.device("cuda"), logger)
    calls = {"fused": 0, "forward": 0}
    clusters = []
    fs, fw, es = tr.model.fused_train_step, tr.model.forward, tr.model.E_step

    def count_fused(*a, **kw):
        calls["fused"] += 1
        return fs(*a, **kw)

    def count_forward(*a, **kw):
        calls["forward"] += 1
        return fw(*a, **kw)

    def record_e_step():
        es()
        clusters.append((tr.model.epoch, tr.model.user_2cluster.clone(), tr.model.user_centroids.clone()))

    tr.model.fused_train_step, tr.model.forward, tr.model.E_step = count_fused, count_forward, record_e_step
    tr.train()
    assert tr.model.fused_step_available() == fused
    assert (calls["fused"] > 0 and calls["forward"] == 0) if fused else (calls["fused"] == 0 and calls["forward"] > 0)
    # the E-step ran at the top of epochs 2 and 3 and found something new the second time
    assert [e for e, _, _ in clusters] == [1, 2]
    assert not torch.equal(clusters[0][1], clusters[1][1]) or not torch.equal(clusters[0][2], clusters[1][2])
    lines = stream.getvalue().splitlines()
    loss_lines = [ln.split("training loss:")[1] for ln in lines if "training loss" in ln]
    recalls = [float(re.search(r"Test recall: \[([^\],]+)", ln).group(1)) for ln in lines if "Test recall" in ln]
    assert len(loss_lines) == 3 and len(recalls) == 3
    for e, ln in enumerate(loss_lines):
        terms = [float(x) for x in ln.split("=")[1].split("+")]
        assert len(terms) == (4 if fused or e > 0 else 3), ln
        assert np.isfinite(terms).all() and np.isfinite(float(ln.split("=")[0]))
        if len(terms) == 4:
            assert (terms[3] == 0.0) if e == 0 else (terms[3] > 0.0), ln  # the prototype term starts with the warm-up's end
    print("recall@20 per epoch", recalls)
    assert recalls[-1] >= recalls[0]
