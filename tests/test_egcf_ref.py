"""tests/egcf_ref64.py — the float64 statement of EGCF's step that tests/test_gpu_egcf.py holds the HIP kernels against —
must BE the reference's step: on egcf_small.npz's dataset files, configuration, initial table and batch it reproduces the
reference's own encoder outputs, three losses and item gradient for both encoders, within the bounds the GPU tests apply
to the same arrays (tests/test_gpu_models.py: test_egcf_vs_reference).  Runs without a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import egcf_ref64 as ref

RTOL = 1e-4  # the suite's bar on losses (tests/test_gpu_models.py)


@pytest.fixture(scope="module")
def egcf_small(tmp_path_factory):
    import utility.utility_data.data_graph as data_graph
    import utility.utility_data.data_loader as data_loader

    eg = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "egcf_small.npz")))
    cfg = dict(zip(eg["config_keys"].tolist(), eg["config_values"].tolist()))
    root = tmp_path_factory.mktemp("egcf_ref")
    d = root / "small"
    d.mkdir()
    (d / "train.txt").write_bytes(eg["train_txt"].tobytes())
    (d / "test.txt").write_bytes(eg["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(root) + "/")
    data = data_loader.Data(str(d), cfg)
    n = data.num_users + data.num_items
    Rm = data_graph.sparse_adjacency_matrix_R(data).tocsr()
    Am = data_graph.sparse_adjacency_matrix(data).tocsr()
    R = ref.dense_operator(Rm.indptr, Rm.indices, Rm.data, (data.num_users, data.num_items))
    A = ref.dense_operator(Am.indptr, Am.indices, Am.data, (n, n))
    return eg, cfg, R, A


@pytest.mark.parametrize("mode", ["parallel", "alternating"])
def test_float64_statement_reproduces_the_reference(egcf_small, mode):
    eg, cfg, R, A = egcf_small
    K, t = int(cfg["GCN_layer"]), float(cfg["temperature"])
    E = torch.from_numpy(eg[mode + "_init_item"])
    with torch.no_grad():
        u, i = ref.egcf_aggregate64(R, A, E.double(), K, mode)
    np.testing.assert_allclose(u.numpy(), eg[mode + "_user"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(i.numpy(), eg[mode + "_item"], rtol=1e-5, atol=1e-7)
    b = torch.from_numpy(eg["batch"])
    losses, dE = ref.egcf_step64(R, A, E, b[:, 0], b[:, 1], b[:, 2], K, mode, float(cfg["reg_lambda"]),
                                 float(cfg["ssl_lambda"]), t)
    np.testing.assert_allclose(losses.numpy(), eg[mode + "_loss"], rtol=RTOL)
    want = eg[mode + "_grad_item"]
    np.testing.assert_allclose(dE.numpy(), want, rtol=1e-3, atol=3e-4 * np.abs(want).max())
    # the float32 composition of the same expressions: the reference's own number format, so closer still
    l32, d32 = ref.egcf_step64(R, A, E, b[:, 0], b[:, 1], b[:, 2], K, mode, float(cfg["reg_lambda"]),
                               float(cfg["ssl_lambda"]), t, dtype=torch.float32)
    e_ref, e_f32 = ref.errors(want, dE, d32)
    print("%s: reference's gradient %.2e, float32 composition %.2e of max |dE| from float64" % (mode, e_ref, e_f32))
    assert l32.dtype == torch.float32 and e_f32 < 1e-4


def test_k1_encoders_coincide(egcf_small):
    """With one layer the two encoders are the same function of the table: a free cross-check of both branches."""
    eg, cfg, R, A = egcf_small
    E = torch.from_numpy(eg["parallel_init_item"])
    b = torch.from_numpy(eg["batch"])
    args = (b[:, 0], b[:, 1], b[:, 2], 1)
    lp, gp = ref.egcf_step64(R, A, E, *args, "parallel", 1e-4, 0.1, 0.1)
    la, ga = ref.egcf_step64(R, None, E, *args, "alternating", 1e-4, 0.1, 0.1)
    # (the dataset's A and R are normalised by two different expressions and each rounded to float32 on its own: their
    #  entries agree to 2^-24 relative, not bit for bit — so do the two encoders, with a layer or two of amplification)
    np.testing.assert_allclose(lp.numpy(), la.numpy(), rtol=1e-6)
    np.testing.assert_allclose(gp.numpy(), ga.numpy(), rtol=0, atol=1e-6 * float(gp.abs().max()))
    # one set of values for both operators: the same function to float64 rounding
    U, I = R.shape
    A2 = torch.zeros_like(A)
    A2[:U, U:], A2[U:, :U] = R, R.t()
    lp, gp = ref.egcf_step64(R, A2, E, *args, "parallel", 1e-4, 0.1, 0.1)
    np.testing.assert_allclose(lp.numpy(), la.numpy(), rtol=1e-12)
    np.testing.assert_allclose(gp.numpy(), ga.numpy(), rtol=0, atol=1e-12 * float(gp.abs().max()))


def test_adam64_is_torch_adam():
    g = torch.Generator().manual_seed(3)
    W = torch.randn(7, 5, generator=g, dtype=torch.float64)
    grads = [torch.randn(7, 5, generator=g, dtype=torch.float64) for _ in range(3)]
    w = torch.nn.Parameter(W.clone())
    opt = torch.optim.Adam([w], lr=1e-3)
    mine = ref.adam64(W, grads, lr=1e-3)
    for k, gk in enumerate(grads):
        w.grad = gk.clone()
        opt.step()
        st = opt.state[w]
        np.testing.assert_allclose(mine[k][0].numpy(), w.detach().numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(mine[k][1].numpy(), st["exp_avg"].numpy(), rtol=1e-13, atol=1e-18)
        np.testing.assert_allclose(mine[k][2].numpy(), st["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-18)
