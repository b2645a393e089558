"""tests/ngcf_ref64.py — the float64 statement of NGCF's layer, training step and message-dropout mask that
tests/test_gpu_ngcf.py holds the kernels against — must BE the reference's: on the golden graph (graph_small.npz, the
normalised adjacency with self loops) and the reference's own weights and batch (next_small.npz) it reproduces the reference's
final panels, losses and gradients, at the tolerances tests/test_gpu_models.py::test_ngcf_vs_reference applies to the same
arrays; and the mask restated in numpy is pinned to splitmix64 and to a scalar restatement in Python integers.  Runs
without a GPU."""
import os

import numpy as np
import torch

from tests import ngcf_ref64 as ref

RTOL = 1e-4  # tests/test_gpu_models.py
REG = 1e-4   # configure/NGCF.txt, what the goldens were taken with
K = 3


def _golden_step(golden_small, dtype):
    g = golden_small
    nx = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "next_small.npz"), allow_pickle=False))
    U, n = int(g["num_users"]), int(g["num_users"]) + int(g["num_items"])
    A = ref.dense_operator(g["adjself_indptr"], g["adjself_indices"], g["adjself_data"], (n, n))
    assert np.array_equal(nx["ngcf_user"][:, :64], nx["ngcf_init_user"])
    E0 = torch.from_numpy(np.concatenate([nx["ngcf_user"][:, :64], nx["ngcf_item"][:, :64]]))
    small = [tuple(torch.from_numpy(nx["ngcf_%s_%d" % (nm, l)]) for nm in ("W_gcn", "b_gcn", "W_bi", "b_bi")) for l in range(K)]
    b = torch.from_numpy(nx["batch"])
    return nx, U, ref.step64(A, E0, small, b[:, 0], b[:, 1], b[:, 2], 0.2, None, REG, U, dtype=dtype)


def test_float64_statement_reproduces_the_references_step(golden_small):
    nx, U, (losses, gE0, gsmall, final) = _golden_step(golden_small, torch.float64)
    assert losses.dtype == torch.float64 and final.dtype == torch.float64 and gE0.dtype == torch.float64
    np.testing.assert_allclose(final[:U].numpy(), nx["ngcf_user"], rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(final[U:].numpy(), nx["ngcf_item"], rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(losses.numpy(), nx["ngcf_loss"], rtol=RTOL)
    np.testing.assert_allclose(gE0[:U].numpy(), nx["ngcf_grad_user"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(gE0[U:].numpy(), nx["ngcf_grad_item"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(gsmall[0][0].numpy(), nx["ngcf_grad_W_gcn_0"], rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(gsmall[2][3].numpy(), nx["ngcf_grad_b_bi_2"], rtol=1e-3, atol=1e-7)
    # the same expressions in float32: the yardstick the GPU file measures the kernels with
    _, _, (l32, g32, s32, f32) = _golden_step(golden_small, torch.float32)
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32 and s32[1][2].dtype == torch.float32
    for name, a, b, c in (("final", nx["ngcf_user"], final[:U], f32[:U]), ("d E0", nx["ngcf_grad_item"], gE0[U:], g32[U:]),
                          ("d W_gcn_0", nx["ngcf_grad_W_gcn_0"], gsmall[0][0], s32[0][0])):
        e_ref, e_f32 = ref.errors(a, b, c)
        print("%s: the reference %.2e, the float32 composition %.2e of max from float64" % (name, e_ref, e_f32))
        assert e_f32 < 1e-5


def test_layer_grads64_is_the_steps_last_layer(golden_small):
    """layer_grads64 with gN = the last slot of d bpr / d final and gE = None gives the step's gradients of layer K's four
    small tensors: the two statements agree (float64, 1e-12 of each tensor's largest entry)."""
    g = golden_small
    nx, U, (losses, gE0, gsmall, final) = _golden_step(g, torch.float64)
    n = final.shape[0]
    A = ref.dense_operator(g["adjself_indptr"], g["adjself_indices"], g["adjself_data"], (n, n))
    small = [tuple(torch.from_numpy(nx["ngcf_%s_%d" % (nm, l)]) for nm in ("W_gcn", "b_gcn", "W_bi", "b_bi")) for l in range(K)]
    ego = final[:, :64]
    for wg, bg, wb, bb in small[:-1]:
        ego, _ = ref.layer64(A @ ego, ego, wg, wb, bg, bb, 0.2, torch.ones(()))
    b = torch.from_numpy(nx["batch"])
    _, gf, _ = ref.bpr64(final, final[:, :64].contiguous(), U, b[:, 0], b[:, 1], b[:, 2], REG, reg_users=False)
    rows = torch.unique(torch.cat([b[:, 0], U + b[:, 1], U + b[:, 2]]))
    poisoned = torch.full((n, 64), float("nan"), dtype=torch.float64)
    poisoned[rows] = gf[rows, 3 * 64:]
    wg, bg, wb, bb = small[-1]
    gT, gs, ge, flat = ref.layer_grads64(A @ ego, ego, wg, wb, bg, bb, 0.2, torch.ones(()), None, poisoned, gn_rows=rows)
    assert torch.isfinite(gT).all() and (gT[~ref._flags(rows, n, "cpu")] == 0).all()
    want = torch.cat([t.reshape(-1) for t in gsmall[-1]])
    for lo, hi in ((0, 4096), (4096, 4160), (4160, 8256), (8256, 8320)):
        assert float((flat[lo:hi] - want[lo:hi]).abs().max()) <= 1e-12 * float(want[lo:hi].abs().max())
    assert torch.equal(flat[4096:4160], flat[8256:8320])  # g b_gcn == g b_bi: both are the column sums of gT
    assert torch.equal(flat[4096:4160], gT.sum(0))


# ------------------------------------------------------------------------------------------------------------ the mask
def _mix64_scalar(seed, stream, row, f4):
    """idg_dropout.h in Python integers."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (stream + 1) + row * 0xBF58476D1CE4E5B9 + f4 * 0x94D049BB133111EB) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_mix64_is_splitmix64():
    # splitmix64 seeded with 0: its state after one step is the golden-ratio constant, its first output this value
    assert int(ref.mix64(0, 0, 0, 0)) == 0xE220A8397B1DCDAF
    assert int(ref.mix64(0, 0, 0, 0)) == _mix64_scalar(0, 0, 0, 0)


def test_vectorised_mix_and_mask_equal_the_scalar_restatement():
    for seed, stream in ((1234, 7), ((1 << 63) + 12345, (1 << 40) + 3)):  # sums that wrap past 2^64 too
        rows, f4 = np.array([0, 1, 65535, 65536, (1 << 31) + 5], dtype=np.int64), np.arange(16, dtype=np.int64)
        got = ref.mix64(seed, stream, rows[:, None], f4[None, :])
        assert got.shape == (5, 16) and got.dtype == np.uint64
        for a, r in enumerate(rows):
            for b, q in enumerate(f4):
                assert int(got[a, b]) == _mix64_scalar(seed, stream, int(r), int(q))
        p = 0.3
        m = ref.keep_mask(p, seed, stream, 5, 16)
        scale = float(np.float32(1) / (np.float32(1) - np.float32(p)))
        assert scale != 1 / (1 - p)  # rounded in float32 first
        for r in range(5):
            for f in range(16):
                bits = (_mix64_scalar(seed, stream, r, f >> 2) >> (16 * (f & 3))) & 0xFFFF
                want = scale if np.float32(bits) * np.float32(2.0 ** -16) >= np.float32(p) else 0.0
                assert float(m[r, f]) == want


def test_mask_properties():
    # a feature's keep bit does not depend on the width
    for p in (0.1, 0.5):
        assert torch.equal(ref.keep_mask(p, 99, 2, 300, 8)[:, :4], ref.keep_mask(p, 99, 2, 300, 4))
        assert torch.equal(ref.keep_mask(p, 99, 2, 300, 100)[:, :7], ref.keep_mask(p, 99, 2, 300, 7))
    assert torch.equal(ref.keep_mask(0.0, 1, 2, 9, 5), torch.ones(9, 5, dtype=torch.float64))
    assert ref.keep_mask(0.3, 1, 2, 9, 5, dtype=torch.float32).dtype == torch.float32
    m = ref.keep_mask(0.3, 1234, 7, 4096, 64)
    dropped = float((m == 0).double().mean())
    print("dropped share at p = 0.3: %.5f" % dropped)
    assert abs(dropped - 0.30242) < 5e-6 and abs(dropped - 0.3) < 0.01
    assert not (m == 0).all(dim=1).any()
    assert set(m.unique().tolist()) == {0.0, ref.keep_scale(0.3)}
    # another stream, another mask
    assert not torch.equal(m, ref.keep_mask(0.3, 1234, 8, 4096, 64))
    # the GPU file's fully dropped rows
    m4 = ref.keep_mask(0.5, 1234, 7, 1000, 4)
    assert int((m4 == 0).all(dim=1).sum()) == 68
    assert ref.keep_scale(0.5) == 2.0


def test_tail64_edges():
    """S2 = None is S2 = 0; a zero row normalises to zero (the clamp), and its Jacobian is I / eps with no projection; the
    LeakyReLU's derivative at exactly 0 is `slope` where kept and 0 where dropped."""
    gen = torch.Generator().manual_seed(3)
    n, d = 6, 8
    S1, b1, b2 = torch.randn(n, d, generator=gen), torch.full((d,), 0.5), torch.full((d,), 0.25)
    S1[2] = -0.75
    S1[4, :3] = -0.75
    mask = ref.keep_mask(0.5, 5, 1, n, d)
    assert (mask[2] == 0).any() and (mask[2] != 0).any()
    E, N = ref.tail64(S1, None, b1, b2, 0.2, mask)
    E2, N2 = ref.tail64(S1, torch.zeros(n, d), b1, b2, 0.2, mask)
    assert torch.equal(E, E2) and torch.equal(N, N2)
    assert (E[2] == 0).all() and (N[2] == 0).all() and (E[4, :3] == 0).all()
    live = E.norm(dim=1) > 0
    np.testing.assert_allclose(N[live].norm(dim=1).numpy(), 1.0, rtol=1e-14)
    gE, gN = torch.randn(n, d, generator=gen, dtype=torch.float64), torch.randn(n, d, generator=gen, dtype=torch.float64)
    gT = ref.tail_grads64(S1, None, b1, b2, 0.2, mask, gE, gN)
    np.testing.assert_allclose(gT[2].numpy(), (0.2 * mask[2] * (gE[2] + gN[2] * 1e12)).numpy(), rtol=1e-14)
    np.testing.assert_allclose(gT[4, :3].numpy(), (0.2 * mask[4, :3] * (gE[4, :3] + gN[4, :3] / E[4].norm())).numpy(), rtol=1e-12)
    only = ref.tail_grads64(S1, None, b1, b2, 0.2, mask, None, gN, gn_rows=[1])
    assert (only[[0, 2, 3, 4, 5]] == 0).all() and (only[1] != 0).any()
