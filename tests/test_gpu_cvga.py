"""CVGA on the GPU: the decoder's fused multinomial NLL and the VAE head against float64 torch, the model against the
reference's goldens, the fused step against the autograd step, determinism at yelp2018 shape, and training end to end.
test_nll_op_over_every_built_width takes its widths from tests/widths.py (EVERY_NK): with them nll_stats_mfma_kernel<NK> and nll_grad_mfma_kernel<NK> run at NK = 3, 5, 6, 7, and every
NK = d / 32 = 1 .. 8 the source builds is held against float64.
Measured on an MI355X (66 tests, 15 s for the whole file; the 24 new cases 0.3 s together): over the new cases the loss within
1.3e-7 relative (bound 1e-5), dZ / dW / dc at most 1.8e-6 / 3.3e-6 / 2.6e-6 of the largest entry (NK = 7, B = 65, I = 3000; bound
1e-5 each)."""
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


@pytest.fixture(scope="module")
def golden_cvga():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "cvga_small.npz")))


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "CVGA.txt"), "CVGA")
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


def _csr(U, I, gen, empty):
    """A train CSR over U users: 0..24 distinct ascending items per row, a few entries of 2 (duplicate edges); the rows
    in `empty` have none."""
    indptr, items, values = [0], [], []
    for u in range(U):
        n = 0 if u in empty else int(gen.integers(1, 25))
        it = np.sort(gen.choice(I, size=min(n, I), replace=False))
        v = np.where(gen.random(len(it)) < 0.15, 2.0, 1.0)
        items.append(it)
        values.append(v)
        indptr.append(indptr[-1] + len(it))
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", t)  # noqa: E731
    return (dev(np.array(indptr), torch.int64), dev(np.concatenate(items), torch.int32),
            dev(np.concatenate(values), torch.float32))


def _nll64(Z, W, c, users, indptr, items, values):
    """The reference's BCE term in float64 (dense x), and its gradients w.r.t. Z, W, c."""
    Z64, W64, c64 = (t.detach().double().requires_grad_(True) for t in (Z, W, c))
    B, I = Z.shape[0], W.shape[0]
    ip, us = indptr.cpu().numpy(), users.cpu().numpy()
    rows = np.repeat(np.arange(B), [int(ip[u + 1] - ip[u]) for u in us])
    x = torch.zeros((B, I), dtype=torch.float64, device="cuda")
    if len(rows):
        sel = torch.from_numpy(np.concatenate([np.arange(ip[u], ip[u + 1]) for u in us])).cuda()
        x[torch.from_numpy(rows).cuda(), items.long()[sel]] = values[sel].double()
    logit = Z64 @ W64.T + c64
    loss = -torch.mean(torch.sum(torch.log_softmax(logit, 1) * x, -1))
    loss.backward()
    return loss.item(), Z64.grad, W64.grad, c64.grad


def _close(mine, ref, tol=1e-5):
    mine, ref = mine.double().cpu().numpy(), ref.double().cpu().numpy()
    np.testing.assert_allclose(mine, ref, rtol=0, atol=tol * max(np.abs(ref).max(), 1e-30))


# --------------------------------------------------------------------------------------- 1. the decoder operator
@pytest.mark.parametrize("d", [32, 48, 64, 128, 256])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 1024])
def test_nll_op_matches_float64_torch(B, d):
    from idgrec_amd import ops

    gen = np.random.default_rng(B * 1000 + d)
    tg = torch.Generator(device="cuda").manual_seed(B * 1000 + d)
    for I in (250, 3000, 38048):
        U = B + 7
        users = torch.from_numpy(gen.permutation(U)[:B]).cuda()
        empty = {int(users[0])} if B > 1 else set()
        indptr, items, values = _csr(U, I, gen, empty)
        Z = torch.randn(B, d, device="cuda", generator=tg) * 0.5
        W = torch.randn(I, d, device="cuda", generator=tg) * 0.3
        c = torch.randn(I, device="cuda", generator=tg) * 0.1
        gZ, gW, gc = torch.full_like(Z, 7.0), torch.full_like(W, 7.0), torch.full_like(c, 7.0)
        loss, _ = ops.multinomial_nll_raw(Z, W, c, users, indptr, items, values, loss=torch.empty(1, device="cuda"),
                                          gZ=gZ, gW=gW, gc=gc)
        ref, rZ, rW, rc = _nll64(Z, W, c, users, indptr, items, values)
        np.testing.assert_allclose(loss.item(), ref, rtol=1e-5)
        _close(gZ, rZ)
        _close(gW, rW)
        _close(gc, rc)
        if empty:  # an empty train row: no gradient
            assert not gZ[0].any()
        # forward only and the autograd op give the same bits
        l2, _ = ops.multinomial_nll_raw(Z, W, c, users, indptr, items, values)
        assert torch.equal(l2, loss)
        Zr, Wr, cr = (t.clone().requires_grad_(True) for t in (Z, W, c))
        la = ops.multinomial_nll(Zr, Wr, cr, users, indptr, items, values)
        (2.0 * la).backward()
        assert torch.equal(la.detach().reshape(1), loss)
        _close(Zr.grad, 2 * rZ)
        _close(cr.grad, 2 * rc)


@pytest.mark.parametrize("I", [250, 3000])
@pytest.mark.parametrize("d", widths.EVERY_NK)
@pytest.mark.parametrize("B", [1, 65, 130])
def test_nll_op_over_every_built_width(B, d, I):
    """The matrix-core forms at NK = d / 32 = 3, 5, 6, 7 (the odd ones leave the last feature block live in half of the waves);
    B = 65 and B = 130 are two and three batch tiles (dW and dc stored by the first, added by the later ones); I = 250 ends
    in a partial item tile.  The body and the bounds of test_nll_op_matches_float64_torch."""
    from idgrec_amd import ops

    seed = 7_000_000 + B * 10_000 + d * 10 + (I > 250)
    gen = np.random.default_rng(seed)
    tg = torch.Generator(device="cuda").manual_seed(seed)
    U = B + 7
    users = torch.from_numpy(gen.permutation(U)[:B]).cuda()
    empty = {int(users[0])} if B > 1 else set()
    indptr, items, values = _csr(U, I, gen, empty)
    Z = torch.randn(B, d, device="cuda", generator=tg) * 0.5
    W = torch.randn(I, d, device="cuda", generator=tg) * 0.3
    c = torch.randn(I, device="cuda", generator=tg) * 0.1
    gZ, gW, gc = torch.full_like(Z, 7.0), torch.full_like(W, 7.0), torch.full_like(c, 7.0)
    loss, _ = ops.multinomial_nll_raw(Z, W, c, users, indptr, items, values, loss=torch.empty(1, device="cuda"),
                                      gZ=gZ, gW=gW, gc=gc)
    ref, rZ, rW, rc = _nll64(Z, W, c, users, indptr, items, values)
    scale = lambda t: max(float(t.abs().max()), 1e-30)  # noqa: E731
    print("NK=%d B=%d I=%d: loss %.2e (relative); dZ %.2e, dW %.2e, dc %.2e of the largest entry (bound 1e-5 each)"
          % (d // 32, B, I, abs(loss.item() - ref) / abs(ref), float((gZ.double() - rZ).abs().max()) / scale(rZ),
             float((gW.double() - rW).abs().max()) / scale(rW), float((gc.double() - rc).abs().max()) / scale(rc)))
    np.testing.assert_allclose(loss.item(), ref, rtol=1e-5)
    _close(gZ, rZ)
    _close(gW, rW)
    _close(gc, rc)
    if empty:  # an empty train row: no gradient
        assert not gZ[0].any()
    # forward only and the autograd op give the same bits
    l2, _ = ops.multinomial_nll_raw(Z, W, c, users, indptr, items, values)
    assert torch.equal(l2, loss)
    Zr, Wr, cr = (t.clone().requires_grad_(True) for t in (Z, W, c))
    la = ops.multinomial_nll(Zr, Wr, cr, users, indptr, items, values)
    (2.0 * la).backward()
    assert torch.equal(la.detach().reshape(1), loss)
    _close(Zr.grad, 2 * rZ)
    _close(Wr.grad, 2 * rW)
    _close(cr.grad, 2 * rc)


def test_nll_op_at_five_million_items():
    from idgrec_amd import ops

    B, I, d = 64, 5_000_000, 64
    gen = np.random.default_rng(5)
    tg = torch.Generator(device="cuda").manual_seed(5)
    users = torch.arange(B, device="cuda")
    indptr, items, values = _csr(B, I, gen, {3})
    Z = torch.randn(B, d, device="cuda", generator=tg) * 0.5
    W = torch.randn(I, d, device="cuda", generator=tg) * 0.3
    c = torch.randn(I, device="cuda", generator=tg) * 0.1
    ws = ops.multinomial_nll_workspace(B, I, d, "cuda")
    assert ws.numel() < 4 * B * I
    gZ, gW, gc = torch.empty_like(Z), torch.empty_like(W), torch.empty_like(c)
    loss, _ = ops.multinomial_nll_raw(Z, W, c, users, indptr, items, values, loss=torch.empty(1, device="cuda"), gZ=gZ,
                                      gW=gW, gc=gc, ws=ws)
    ref, rZ, rW, rc = _nll64(Z, W, c, users, indptr, items, values)
    np.testing.assert_allclose(loss.item(), ref, rtol=1e-5)
    _close(gZ, rZ)
    _close(gW, rW)
    _close(gc, rc)


def test_nll_op_is_bit_reproducible():
    from idgrec_amd import ops

    B, I, d = 1024, 38048, 64
    gen = np.random.default_rng(9)
    tg = torch.Generator(device="cuda").manual_seed(9)
    users = torch.from_numpy(gen.permutation(B)).cuda()
    indptr, items, values = _csr(B, I, gen, {5})
    Z, W = torch.randn(B, d, device="cuda", generator=tg), torch.randn(I, d, device="cuda", generator=tg) * 0.2
    c = torch.randn(I, device="cuda", generator=tg) * 0.1
    out = []
    for _ in range(2):
        g = (torch.empty_like(Z), torch.empty_like(W), torch.empty_like(c))
        loss, _ = ops.multinomial_nll_raw(Z, W, c, users, indptr, items, values, loss=torch.empty(1, device="cuda"),
                                          gZ=g[0], gW=g[1], gc=g[2])
        out.append((loss,) + g)
    for a, b in zip(*out):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------- 2. the head
@pytest.mark.parametrize("d", [48, 64])
def test_head_matches_float64_torch(d):
    from idgrec_amd import ops

    B, U, p = 300, 1000, 0.3
    tg = torch.Generator(device="cuda").manual_seed(d)
    panel = torch.randn(U, 2 * d, device="cuda", generator=tg) * 0.5
    bias = torch.randn(2 * d, device="cuda", generator=tg) * 0.1
    users = torch.randperm(U, device="cuda", generator=tg)[:B]
    eps_out = torch.empty(B, d, device="cuda")
    keep = torch.empty(B, 2 * d, device="cuda")
    z, kl = ops.vae_head_raw(panel, users, bias, p, 11, 5, pre_rows=users, eps_out=eps_out, keep_out=keep)
    assert set(torch.unique(keep).tolist()) <= {0.0, float(np.float32(1.0) / np.float32(1.0 - p))}
    pre64 = panel[users].double().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    h = keep.double() * (pre64 + b64)
    mu, lv = h[:, :d], h[:, d:]
    z64 = eps_out.double() * torch.exp(0.5 * lv) + mu
    kl64 = -0.5 / B * torch.mean(torch.sum(1 + lv - mu.pow(2) - lv.exp(), dim=1))
    _close(z, z64.detach())
    np.testing.assert_allclose(kl.item(), kl64.item(), rtol=1e-5)
    gz = torch.randn(B, d, device="cuda", generator=tg)
    ((z64 * gz.double()).sum() + 3.0 * kl64).backward()
    gpre = torch.full_like(panel, 9.0)
    gbias = torch.empty_like(bias)
    ops.vae_head_bwd_raw(panel, users, bias, p, 11, 5, gz, gpre, upstream_kl=torch.tensor([3.0], device="cuda"),
                         gbias=gbias, pre_rows=users, gpre_rows=users)
    _close(gpre[users], pre64.grad)
    _close(gbias, b64.grad)
    # the backward regenerated the forward's mask: exactly the dropped features have a zero gradient
    assert torch.equal(gpre[users] == 0, keep == 0)
    rest = torch.ones(U, dtype=torch.bool, device="cuda")
    rest[users] = False
    assert bool((gpre[rest] == 9.0).all())
    # injected eps: the same z; without the KL output (a NULL kl for the library): the same z again
    z2, _ = ops.vae_head_raw(panel, users, bias, p, 11, 5, pre_rows=users, eps=eps_out)
    assert torch.equal(z2, z)
    z3, kl3 = ops.vae_head_raw(panel, users, bias, p, 11, 5, pre_rows=users, with_kl=False)
    assert kl3 is None and torch.equal(z3, z)


def test_head_noise_and_mask_statistics():
    from idgrec_amd import ops

    B, d, p = 8192, 64, 0.3
    pre = torch.zeros(B, 2 * d, device="cuda")
    users = torch.arange(B, device="cuda")
    eps = torch.empty(B, d, device="cuda")
    keep = torch.empty(B, 2 * d, device="cuda")
    ops.vae_head_raw(pre, users, torch.zeros(2 * d, device="cuda"), p, 2024, 1, eps_out=eps, keep_out=keep)
    e = torch.cat([eps.flatten(), ops.vae_head_raw(pre, users, torch.zeros(2 * d, device="cuda"), 0.0, 2024, 2,
                                                   eps_out=torch.empty(B, d, device="cuda"))[0].flatten()]).double()
    n = e.numel()
    assert n >= 1_000_000
    assert abs(e.mean().item()) < 5 / np.sqrt(n)
    assert abs(e.var().item() - 1) < 5 * np.sqrt(2 / n)
    rate = (keep != 0).double().mean().item()
    assert abs(rate - (1 - p)) < 5 * np.sqrt(p * (1 - p) / keep.numel())


# --------------------------------------------------------------------------------------- 3. the model vs the reference
def _model(cfg, data):
    import utility.utility_function.tools as tools
    from models.CVGA import CVGA

    tools.set_seed(2024)
    return CVGA(cfg, data, torch.device("cuda")).to("cuda")


def _tensors(m):
    return [m.q_layers[0].weight, m.q_layers[0].bias, m.p_layers[0].weight, m.p_layers[0].bias]


NAMES = ("wq", "bq", "wp", "c")


def test_model_matches_reference_goldens(tmp_path, golden_small, golden_cvga):
    g = golden_cvga
    cfg = _cfg(dropout=0, batch_size=96)
    data = _small_data(tmp_path, golden_small, cfg)
    m = _model(cfg, data)
    for name, t in zip(NAMES, _tensors(m)):
        assert np.array_equal(t.detach().cpu().numpy(), g["init_" + name]), name
    assert m.q_layers[0].weight.t().is_contiguous()
    users = torch.from_numpy(g["batch_users"]).cuda()
    ll = m(users, None, eps=torch.from_numpy(g["batch_eps"]).cuda())
    np.testing.assert_allclose([x.item() for x in ll], g["batch_loss"], rtol=1e-5)
    sum(ll).backward()
    for name, t in zip(NAMES, _tensors(m)):
        ref = g["grad_" + name]
        np.testing.assert_allclose(t.grad.cpu().numpy(), ref, rtol=0, atol=1e-5 * np.abs(ref).max(), err_msg=name)
    # encode() keeps the reference's meaning: (mu, logvar) of every user; with the golden eps they give the head's z
    m.eval()
    with torch.no_grad():
        mu, logvar = m.encode()
        z_ref = torch.from_numpy(g["batch_eps"]).cuda() * torch.exp(0.5 * logvar[users]) + mu[users]
        z_head, _ = m.encode_z(users, eps=torch.from_numpy(g["batch_eps"]).cuda())
    assert mu.shape == logvar.shape == (data.num_users, int(cfg["embedding_size"]))
    np.testing.assert_allclose(z_head.cpu().numpy(), z_ref.cpu().numpy(), rtol=1e-6, atol=1e-6)
    # evaluation: dense logits and top-K with the reference's eps
    ru = torch.from_numpy(g["rating_users"]).cuda()
    reps = torch.from_numpy(g["rating_eps"]).cuda()
    R = m.get_rating_for_test(ru, eps=reps).cpu().numpy()
    tol = 1e-5 * np.abs(g["rating"]).max()
    np.testing.assert_allclose(R, g["rating"], rtol=0, atol=tol)
    k = 20
    top = m.topk_for_test(ru, k, eps=reps).cpu().numpy()
    masked = g["rating"].copy()
    for r, u in enumerate(g["rating_users"]):
        masked[r, data.all_positive[u]] = -1
    for r in range(len(ru)):
        order = np.argsort(-masked[r], kind="stable")
        srt = masked[r][order]
        for j in range(k):
            gap = min(srt[j] - srt[j + 1], srt[j - 1] - srt[j] if j else np.inf)
            if gap > 2 * tol:
                assert top[r, j] == order[j], (r, j)


def test_fused_adam_steps_match_reference_trajectory(tmp_path, golden_small, golden_cvga):
    g = golden_cvga
    cfg = _cfg(dropout=0, batch_size=96)
    data = _small_data(tmp_path, golden_small, cfg)
    m = _model(cfg, data)
    opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    order = torch.from_numpy(g["order"]).cuda()
    loss = torch.zeros((3, 2), device="cuda")
    for s in range(3):
        assert m.fused_train_step(order[s * 96:(s + 1) * 96], loss[s], opt, eps=torch.from_numpy(g["traj_eps"][s]).cuda())
        # (Adam divides by sqrt(v): where a gradient is of the order of its own rounding error a last-place difference
        # moves the element by up to a step's reach — the criterion of the DirectAU trajectory check)
        for name, t in zip(NAMES, _tensors(m)):
            mine, ref = t.detach().cpu().numpy(), g["traj%d_%s" % (s, name)]
            off = ~np.isclose(mine, ref, rtol=1e-4, atol=1e-6)
            assert off.mean() < 1e-3, (s, name, off.mean())
            assert np.abs(mine - ref).max() < 1e-4, (s, name, np.abs(mine - ref).max())
    np.testing.assert_allclose(loss.cpu().numpy(), g["traj_loss"], rtol=1e-5)


# --------------------------------------------------------------------------------------- 4. fused step == autograd step
def test_fused_step_equals_autograd_step(tmp_path, golden_small):
    from idgrec_amd import ops

    cfg = _cfg(dropout=0.3, batch_size=96)
    data = _small_data(tmp_path, golden_small, cfg)
    batches = [torch.arange(s * 96, (s + 1) * 96, device="cuda") for s in range(3)]
    res = []
    for fused in (True, False):
        m = _model(cfg, data)
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=0.001)
        loss = torch.zeros((3, 2), device="cuda")
        for s in range(3):
            stream = (2024, 100 + s)
            if fused:
                m.fused_loss_and_grad(batches[s], loss[s], stream=stream)
            else:
                users = batches[s]
                pre = ops.encode_rows(m.Graph, m.q_layers[0].weight.t(), users)
                z, kl = ops.vae_head(pre, m.q_layers[0].bias, users, m.dropout, stream=stream)
                ip, ix, iv = m._train_csr()
                recon = ops.multinomial_nll(z, m.p_layers[0].weight, m.p_layers[0].bias, users, ip, ix, iv)
                loss[s] = torch.stack([recon.detach(), kl.detach()])
                opt.zero_grad()
                (recon + kl).backward()
            grads = [t.grad.clone() for t in _tensors(m)]
            opt.step()
        res.append((loss.cpu().numpy(), [t.detach().cpu().numpy() for t in _tensors(m)], [x.cpu().numpy() for x in grads]))
    (l_f, w_f, g_f), (l_a, w_a, g_a) = res
    np.testing.assert_allclose(l_f, l_a, rtol=2e-5)
    for a, b in zip(g_f, g_a):
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5 * np.abs(b).max())
    for a, b in zip(w_f, w_a):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)


# --------------------------------------------------------------------------------------- 5. yelp2018 shape
def test_fused_training_is_bit_reproducible_at_yelp_shape(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    from idgrec_amd import ops

    S.make_dataset(str(tmp_path), "yelp2018", n_test=1)
    cfg = _cfg(dataset="yelp2018", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "yelp2018"), cfg)
    order = torch.from_numpy(np.random.default_rng(0).permutation(data.num_users)).cuda()
    out = []
    for run in range(2):
        ops.reset_noise_stream(0)
        m = _model(cfg, data)
        opt = torch.optim.Adam(m.parameters(), lr=0.001)
        loss = torch.zeros((20, 2), device="cuda")
        for s in range(20):
            assert m.fused_train_step(order[s * 1024:(s + 1) * 1024], loss[s], opt)
        out.append([t.detach().clone() for t in _tensors(m)] + [loss.clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out[0][-1]).all())


# --------------------------------------------------------------------------------------- 6. end to end
def test_training_curve_lies_in_the_reference_band(tmp_path):
    """31 epochs on medium_conv with configure/CVGA.txt's dropout 0.3, learning rate and batch size, through the trainer,
    against three seeds of the reference's own run (cvga_curve_medium.npz).  The port draws its dropout mask and eps from
    a counter-based generator, not torch's stream, so it is one more sample of the reference's run-to-run spread, not a
    replay of one run.  Margin: that spread, pooled over the tested epochs as a relative standard deviation s (sample
    variance of value / seed-mean, 2 degrees of freedom per epoch: 14 for Recall@20, 62 for the loss; measured s = 7.2 %
    and 0.099 %), times 3, added on both sides of the seeds' [min, max] at each epoch — with min and max of three
    samples about 0.85 s from their mean, the band is the seed mean +- ~3.9 s, so one honest run leaves it at one epoch of
    seven with a probability well below 1 %; a systematic deviation of the size of the spread itself does not pass."""
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "cvga_curve_medium.npz")))
    src = os.path.join(ROOT, "tests", "golden", "inputs", "medium_conv")
    d = tmp_path / "medium"
    d.mkdir()
    for f in ("train.txt", "test.txt"):
        (d / f).write_bytes(open(os.path.join(src, f), "rb").read())
    ref_cfg = dict(zip(g["config_keys"].tolist(), g["config_values"].tolist()))
    cfg = _cfg(dataset="medium", dataset_path=str(tmp_path) + "/", training_epochs=31, interval=5, early_stopping=1000)
    for k in ("dropout", "learn_rate", "batch_size", "embedding_size", "top_K", "test_batch_size", "training_epochs", "interval"):
        assert cfg[k] == ref_cfg[k], k
    stream = io.StringIO()
    logger = logging.getLogger("cvga_curve")
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(int(g["seeds"][0]))
    data = data_loader.Data(str(d), cfg)
    tr = importlib.import_module("models.CVGA").Trainer(None, cfg, data, torch.device("cuda"), logger)
    tr.train()
    lines = stream.getvalue().splitlines()
    loss = np.array([_numbers(ln.split("training loss:")[1]) for ln in lines if "training loss" in ln])
    tests = [ln for ln in lines if "Test recall" in ln]
    assert [int(_numbers(ln.split("|")[0])[0]) for ln in tests] == g["test_epochs"].tolist()
    recall = np.array([_numbers(ln.split("Test recall:")[1].split("|")[0]) for ln in tests])

    def band(ref, mine, what):
        mean = ref.mean(0)
        s = np.sqrt((((ref / mean) - 1) ** 2).sum() / (ref.shape[1] * (ref.shape[0] - 1)))
        lo, hi = ref.min(0) - 3 * s * mean, ref.max(0) + 3 * s * mean
        out = (mine < lo) | (mine > hi)
        assert not out.any(), (what, s, np.nonzero(out)[0].tolist(), mine[out].tolist(), lo[out].tolist(), hi[out].tolist())

    band(g["recall"][:, :, 0], recall[:, 0], "Recall@20")
    band(g["loss"][:, :, 0], loss[:, 0], "total loss")



def _numbers(text):
    return [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", text)]


@pytest.mark.parametrize("d", [64, 48])
def test_trainer_end_to_end(d, tmp_path, golden_small):
    import utility.utility_function.tools as tools

    cfg = _cfg(embedding_size=d, training_epochs=3, interval=1, batch_size=96, top_K="[20, 40]", test_batch_size=64,
               learn_rate=0.01)
    data = _small_data(tmp_path, golden_small, cfg)
    stream = io.StringIO()
    logger = logging.getLogger("cvga_e2e_%d" % d)
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.StreamHandler(stream)]
    tools.set_seed(2024)
    tr = importlib.import_module("models.CVGA").Trainer(None, cfg, data, torch.device("cuda"), logger)
    tr.train()
    assert tr.model.fused_step_available()
    lines = stream.getvalue().splitlines()
    loss_lines = [ln for ln in lines if "training loss" in ln]
    assert len(loss_lines) == 3
    totals = []
    for ln in loss_lines:
        assert re.fullmatch(r"Epoch: +\d+ \| Training time: \d+\.\d{3} \| training loss: \S+ = \S+ \+ \S+", ln), ln
        t, r, k = _numbers(ln.split("training loss:")[1])
        assert abs(t - (r + k)) < 1e-4 and np.isfinite([r, k]).all()
        totals.append(t)
    # (the loss of one epoch carries the noise of eps and of the dropout mask: only the trend over the three is checked)
    assert totals[2] < totals[0], totals
    tests = [ln for ln in lines if "Test recall" in ln]
    assert len(tests) == 3
    assert re.fullmatch(r"Best epoch: +\d+ \| Best recall: \[.*\] \| Best NDCG: \[.*\]", lines[-1]), lines[-1]
    assert lines[-2] == "Model training process completed."
