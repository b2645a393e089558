"""tests/bpr_ref64.py — the float64 statement of the BPR loss pair, its gradients and the row-masked Adam step that
tests/test_gpu_bpr.py holds idg_bpr.hip's kernels against — must BE the reference's: on the golden graphs' panels and
batch it reproduces the reference's own losses and gradients for LightGCN (final panel and ego panel apart) and MFBPR (one
panel), at the tolerance the GPU tests apply to the same arrays (tests/test_gpu_parity.py: RTOL).  Runs without a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import bpr_ref64 as ref

RTOL = 1e-4  # tests/test_gpu_parity.py
REG = 1e-4   # the reg_lambda the goldens were taken with (tests/test_gpu_parity.py passes the same)


def _panels(g):
    fin = torch.from_numpy(np.concatenate([g["d64_lgcn_user"], g["d64_lgcn_item"]]))
    ego = torch.from_numpy(np.concatenate([g["d64_init_user"], g["d64_init_item"]]))
    b = torch.from_numpy(g["d64_batch"])
    return fin, ego, int(g["num_users"]), b[:, 0], b[:, 1], b[:, 2]


@pytest.mark.parametrize("gname", ["small", "tiny"])
def test_float64_statement_reproduces_lightgcn_loss_and_gradients(gname, golden_small, golden_tiny):
    """Losses: d64_lgcn_loss.  Gradients: the reference's table gradient d64_lgcn_grad_* is  P^T . (d bpr / d final) +
    d reg / d ego  with P the layer mean of the normalised adjacency, and the golden files keep its ingredients:
    d64_lgcn_gfinal_* is d bpr / d final (bpr64's first gradient is pinned to it) and d64_lgcn_gbpr_* is that gradient
    after the propagation's backward, so that  d64_lgcn_gbpr_* + (bpr64's second gradient)  must give d64_lgcn_grad_*."""
    g = golden_small if gname == "small" else golden_tiny
    fin, ego, U, users, pos, neg = _panels(g)
    losses, gf, ge = ref.bpr64(fin, ego, U, users, pos, neg, REG)
    assert losses.dtype == torch.float64
    np.testing.assert_allclose(losses.numpy(), g["d64_lgcn_loss"], rtol=RTOL)
    want_f = np.concatenate([g["d64_lgcn_gfinal_user"], g["d64_lgcn_gfinal_item"]])
    np.testing.assert_allclose(gf.numpy(), want_f, rtol=RTOL, atol=1e-8)
    through = np.concatenate([g["d64_lgcn_gbpr_user"], g["d64_lgcn_gbpr_item"]]).astype(np.float64)
    total = np.concatenate([g["d64_lgcn_grad_user"], g["d64_lgcn_grad_item"]]).astype(np.float64)
    np.testing.assert_allclose(through + ge.numpy(), total, rtol=RTOL, atol=1e-8)
    l32, gf32, ge32 = ref.bpr64(fin, ego, U, users, pos, neg, REG, dtype=torch.float32)
    assert l32.dtype == torch.float32 and gf32.dtype == torch.float32
    e_ref, e_f32 = ref.errors(want_f, gf, gf32)
    print("%s: reference's d bpr / d final %.2e, float32 composition %.2e of max from float64" % (gname, e_ref, e_f32))
    assert e_f32 < 1e-5


@pytest.mark.parametrize("gname", ["small", "tiny"])
def test_float64_statement_reproduces_mfbpr_loss_and_gradients(gname, golden_small, golden_tiny):
    """`fin is ego`: d64_mf_loss and d64_mf_grad_*, the one panel receiving both gradients."""
    g = golden_small if gname == "small" else golden_tiny
    _, W, U, users, pos, neg = _panels(g)
    losses, gf, ge = ref.bpr64(W, W, U, users, pos, neg, REG)
    assert gf is ge
    np.testing.assert_allclose(losses.numpy(), g["d64_mf_loss"], rtol=RTOL)
    np.testing.assert_allclose(gf[:U].numpy(), g["d64_mf_grad_user"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(gf[U:].numpy(), g["d64_mf_grad_item"], rtol=RTOL, atol=1e-8)
    # the one panel's gradient is the sum of the two the separate-panel form returns
    W2 = W.clone()
    l2, gf2, ge2 = ref.bpr64(W, W2, U, users, pos, neg, REG)
    np.testing.assert_allclose(l2.numpy(), losses.numpy(), rtol=1e-14)
    np.testing.assert_allclose((gf2 + ge2).numpy(), gf.numpy(), rtol=1e-12, atol=1e-18)


def test_item_only_regulariser_reproduces_ngcf_loss_pair_and_is_the_full_one_minus_the_user_block():
    """reg_users=False.  next_small.npz (what test_ngcf_vs_reference reads) holds NGCF's loss pair, its batch and the
    256-wide final panels, whose first 64 columns ARE the ego rows (layer 0 of the concatenation: checked against
    ngcf_init_user below) — so the LOSS PAIR is pinned against the reference's own numbers, at widths (256, 64).  Its
    gradients are the whole model's (through three layers and their weights), not this function's: for those, the
    identity  reg_users=False  ==  reg_users=True minus the user block's term and gradient rows  is asserted instead."""
    nx = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "next_small.npz"), allow_pickle=False))
    fin = torch.from_numpy(np.concatenate([nx["ngcf_user"], nx["ngcf_item"]]))
    U = nx["ngcf_user"].shape[0]
    assert np.array_equal(nx["ngcf_user"][:, :64], nx["ngcf_init_user"])
    ego = fin[:, :64].contiguous()
    b = torch.from_numpy(nx["batch"])
    users, pos, neg = b[:, 0], b[:, 1], b[:, 2]
    losses, gf, ge = ref.bpr64(fin, ego, U, users, pos, neg, REG, reg_users=False)
    np.testing.assert_allclose(losses.numpy(), nx["ngcf_loss"], rtol=RTOL)
    assert gf.shape == fin.shape and ge.shape == ego.shape
    assert (ge[:U] == 0).all()
    full, gf_full, ge_full = ref.bpr64(fin, ego, U, users, pos, neg, REG, reg_users=True)
    B = users.shape[0]
    user_term = REG * 0.5 * (ego[users].double() ** 2).sum() / B
    np.testing.assert_allclose(float(losses[0]), float(full[0]), rtol=1e-14)
    np.testing.assert_allclose(float(losses[1]), float(full[1] - user_term), rtol=1e-12)
    assert torch.equal(gf, gf_full)
    np.testing.assert_allclose(ge[U:].numpy(), ge_full[U:].numpy(), rtol=1e-14)
    counts = torch.bincount(users, minlength=U).double()
    np.testing.assert_allclose(ge_full[:U].numpy(), (REG / B * counts[:, None] * ego[:U].double()).numpy(), rtol=1e-12, atol=1e-20)


def test_upstream_scalars_scale_the_two_gradients(golden_small):
    fin, ego, U, users, pos, neg = _panels(golden_small)
    l1, gf1, ge1 = ref.bpr64(fin, ego, U, users, pos, neg, REG)
    l2, gf2, ge2 = ref.bpr64(fin, ego, U, users, pos, neg, REG, upstream=(2.0, -3.0))
    assert torch.equal(l1, l2)
    np.testing.assert_allclose(gf2.numpy(), 2.0 * gf1.numpy(), rtol=1e-14)
    np.testing.assert_allclose(ge2.numpy(), -3.0 * ge1.numpy(), rtol=1e-14)


def test_adam_rows64_is_torch_adam_on_a_masked_gradient():
    """adam64 plus the row mask against torch.optim.Adam in float64 fed the gradient with the unflagged rows zeroed; the
    rows' bits change between steps, so a row's moments decay while its gradient is absent.  What the statement is
    handed at the unflagged rows (NaN here) is not read."""
    gen = torch.Generator().manual_seed(5)
    n, d = 40, 8
    W = torch.randn(n, d, generator=gen, dtype=torch.float64)
    grads = [torch.randn(n, d, generator=gen, dtype=torch.float64) for _ in range(3)]
    bits = [torch.rand(n, generator=gen) < 0.5 for _ in range(3)]
    assert any((bits[0] & ~bits[1]).tolist()) and any((~bits[0] & bits[1]).tolist())
    w = torch.nn.Parameter(W.clone())
    opt = torch.optim.Adam([w], lr=1e-3)
    poisoned = [torch.where(b[:, None], g, torch.full_like(g, float("nan"))) for g, b in zip(grads, bits)]
    mine = ref.adam_rows64(W, poisoned, bits, lr=1e-3)
    for k, (gk, bk) in enumerate(zip(grads, bits)):
        w.grad = gk * bk[:, None].double()
        opt.step()
        st = opt.state[w]
        # (two float64 evaluations of one recurrence: torch forms exp_avg as M + (g - M) * (1 - beta1), a few roundings
        #  of the LARGER of |g|, |M| away from beta1 * M + (1 - beta1) * g — an absolute distance, 1e-14 of the largest entry)
        np.testing.assert_allclose(mine[k][0].numpy(), w.detach().numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(mine[k][1].numpy(), st["exp_avg"].numpy(), rtol=1e-13, atol=1e-14 * float(st["exp_avg"].abs().max()))
        np.testing.assert_allclose(mine[k][2].numpy(), st["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-14 * float(st["exp_avg_sq"].abs().max()))
    dropped = bits[0] & ~bits[1]  # a gradient at step 1, none at step 2: the moments decayed, the row still moved
    assert (mine[1][1][dropped] == 0.9 * mine[0][1][dropped]).all()
    assert (mine[1][0][dropped] != mine[0][0][dropped]).all()
