"""tests/ssl_ref64.py — the float64 statement that tests/test_gpu_ssl.py holds the noise epilogues, idg_propagate_views_f32
and the engine's `ssl` / `xssl` / `sgl` steps against — checked without a GPU: its Philox4x32-10 reproduces the published
known-answer vectors, its uniforms are what the contract says, with epsilon = 0 its three steps ARE the reference's
(tests/golden/next_small.npz), and at every case of the GPU file no layer output has an entry so close to zero that a float32
product could take the other sign (fragile() == 0: the GPU comparisons then leave nothing out)."""
import os

import numpy as np
import pytest
import torch

from tests import ssl_ref64 as ref


@pytest.fixture(scope="module")
def golden_next():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "next_small.npz")))


@pytest.fixture(scope="module")
def operators(golden_small):
    out = {}
    for name, (ip, ix, dv, n, U) in (("small", ref.small_graph(golden_small)), ("hub", ref.hub_graph())):
        out[name] = (ref.dense_operator(ip, ix, dv, (n, n)), n, U)
    return out


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert tuple(int(x) for x in ref.philox4x32_10(ctr, key)) == want
    # broadcast: the same block inside an array of counters
    got = ref.philox4x32_10((np.array([1, ctr[0]]), ctr[1], ctr[2], ctr[3]), key)
    assert tuple(int(x[1]) for x in np.broadcast_arrays(*got)) == want


def test_uniforms_follow_the_contract():
    seed, sid = (0xABCD << 32) | 99, (3 << 32) | 7
    u = ref.uniforms(seed, sid, 300, 100)
    assert u.shape == (300, 100) and u.min() >= 0 and u.max() < 1
    assert np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))  # multiples of 2^-24
    assert abs(u.mean() - 0.5) < 0.01 and abs(u.var() - 1 / 12) < 0.005
    # word j of block b of row r is feature 4b + j; a narrower table is a prefix (the norm, not the draw, depends on d)
    w = ref.philox4x32_10((17, 0, 5, 7), (99, 0xABCD ^ 3))
    assert np.array_equal(u[17, 20:24], [(int(x) >> 8) * 2.0 ** -24 for x in w])
    assert np.array_equal(ref.uniforms(seed, sid, 300, 7), u[:, :7])
    assert np.array_equal(ref.uniforms(seed, sid, 2, 100, rows=[17, 299]), u[[17, 299]])
    # a row beyond 2^32 differs from its low word (counter word 1)
    assert not np.array_equal(ref.uniforms(seed, sid, 1, 8, rows=[(1 << 32) + 17]), u[17:18, :8])
    # distinct (seed, stream, row, block) give distinct draws: no block of any of these tables occurs twice
    tables = [u, ref.uniforms(seed, 7, 300, 100), ref.uniforms(seed, sid + 1, 300, 100), ref.uniforms(99, sid, 300, 100),
              ref.uniforms(seed ^ (1 << 40), sid, 300, 100), ref.uniforms(seed, ref.substream(sid, 0), 300, 100)]
    blocks = np.concatenate([t.reshape(-1, 4) for t in tables])
    assert len(np.unique(blocks, axis=0)) == len(blocks)
    assert not np.array_equal(tables[0], tables[1])  # (3 << 32) | 7 is not 7
    # the high word of the stream and of the seed meet in ONE key word: (seed_hi, stream_hi) and (stream_hi, seed_hi) coincide
    # there — part of the contract (include/idgrec.h), stated here so that a change of it is seen
    assert np.array_equal(ref.uniforms((5 << 32) | 1, (9 << 32) | 2, 4, 8), ref.uniforms((9 << 32) | 1, (5 << 32) | 2, 4, 8))
    assert ref.substream((1 << 58) + 3, 2) == 3 * 64 + 2  # sid * 64 wraps as in uint64_t


def test_perturbation_moves_each_row_by_eps_along_its_signs():
    X = ref.table(50, 48, 4).double()
    X[7] = 0
    X[9, :5] = 0
    Y = ref.perturb64(X, 0.3, 11, 12)
    delta = Y - X
    moved = torch.ones(50, dtype=torch.bool)
    moved[[7, 9]] = False
    np.testing.assert_allclose(delta[moved].norm(dim=1).numpy(), 0.3, rtol=1e-12)
    assert bool((delta * torch.sign(X) >= 0).all()) and bool((delta[7] == 0).all()) and bool((delta[9, :5] == 0).all())
    assert float(delta[9].norm()) < 0.3  # the norm runs over all 48 draws, also where sign() is 0
    u = torch.from_numpy(ref.uniforms(11, 12, 50, 48))
    np.testing.assert_allclose((delta[3] / torch.sign(X[3])).numpy(), (u[3] / u[3].norm() * 0.3).numpy(), rtol=1e-12)


def test_views_take_the_sub_streams_of_their_entry_points(operators):
    """The stream table of the module docstring, stated once by hand: the shared-first-product passes draw sid * 64 + (k - 1),
    idg_propagate_mean_noise_f32 draws sid * 64 + k."""
    A, n, U = operators["small"]
    E0, eps, seed, sid = ref.table(n, 64, 1).double(), 0.1, 77, 6
    x1 = ref.perturb64(A @ E0, eps, seed, sid * 64)
    x2 = ref.perturb64(A @ x1, eps, seed, sid * 64 + 1)
    x3 = ref.perturb64(A @ x2, eps, seed, sid * 64 + 2)
    clean, view = ref.views64(A, E0, 3, False, eps, [(seed, sid)])
    assert torch.equal(view, torch.stack([x1, x2, x3], dim=1).mean(dim=1))
    assert torch.equal(clean, ref.propagate_clean64(A, E0, 3, False))
    y1 = ref.perturb64(A @ E0, eps, seed, sid * 64 + 1)
    y2 = ref.perturb64(A @ y1, eps, seed, sid * 64 + 2)
    assert torch.equal(ref.propagate_noise64(A, E0, 2, True, eps, seed, sid, 1), torch.stack([E0, y1, y2], dim=1).mean(dim=1))
    # layer 0 in the mean, one layer, or a width without tiled kernels: every view is idg_propagate_mean_noise_f32's
    assert torch.equal(ref.views64(A, E0, 2, True, eps, [(seed, sid)])[1], torch.stack([E0, y1, y2], dim=1).mean(dim=1))
    assert torch.equal(ref.views64(A, E0, 1, False, eps, [(seed, sid)])[1], y1)
    E48 = E0[:, :48].contiguous()
    assert torch.equal(ref.views64(A, E48, 2, False, eps, [(seed, sid)])[1], ref.propagate_noise64(A, E48, 2, False, eps, seed, sid, 1))


# ------------------------------------------------------------------------------------------------ the reference's numbers
def _anchor(golden_small, golden_next, operators, name, tag):
    g, nx = golden_small, golden_next
    A, n, U = operators["small"]
    E0 = torch.from_numpy(np.concatenate([g["d64_init_user"], g["d64_init_item"]]))
    b = torch.from_numpy(nx["batch"])
    mats = [A]
    if name == "SGL":
        mats += [ref.dense_operator(nx[k + "_indptr"], nx[k + "_indices"], nx[k + "_data"], (n, n)) for k in ("sgl_sub1", "sgl_sub2")]
        cfg = ref.read_config(name)
    else:
        cfg = ref.read_config(name, epsilon=0.0)
    out = {}
    for dtype in (torch.float64, torch.float32):
        losses, dE = ref.engine_step64(name, mats, E0, U, (b[:, 0], b[:, 1], b[:, 2]), cfg, 1, dtype)
        assert losses.dtype == dtype
        out[dtype] = (losses.double().numpy(), dE.double().numpy())
    want_l, want_g = nx[tag + "_loss"], np.concatenate([nx[tag + "_grad_user"], nx[tag + "_grad_item"]]).astype(np.float64)
    e64 = np.abs(out[torch.float64][1] - want_g).max() / np.abs(want_g).max()
    e32 = np.abs(out[torch.float32][1] - out[torch.float64][1]).max() / np.abs(want_g).max()
    e_both = np.abs(out[torch.float32][1] - want_g).max() / np.abs(want_g).max()
    print("%s: losses %.2e relative; the reference's gradient %.2e of max |ref| from the float64 statement, the float32 "
          "statement %.2e from the float64 one and %.2e from the reference's" % (name, np.abs(out[torch.float64][0] / want_l - 1).max(), e64, e32, e_both))
    np.testing.assert_allclose(out[torch.float64][0], want_l, rtol=1e-5)
    return e64, e32


@pytest.mark.parametrize("name", ["SimGCL", "XSimGCL"])
def test_steps_with_epsilon_zero_are_the_references(name, golden_small, golden_next, operators):
    """simgcl0_* / xsimgcl0_* of next_small.npz (what test_ssl_step_with_epsilon_zero_vs_reference reads): losses rtol 1e-5,
    gradients within 1e-5 of the largest entry — the goldens are float32 runs."""
    e64, e32 = _anchor(golden_small, golden_next, operators, name, name.lower() + "0")
    assert e64 <= 1e-5 and e32 <= 1e-5


SGL_MEASURED = 9.91e-5


def test_sgl_step_is_the_references(golden_small, golden_next, operators):
    """sgl_* of next_small.npz (what test_sgl_three_views_vs_reference reads, there at atol 3e-4 of max |ref|).  Measured: the
    reference's gradient sits 9.90e-5 of its largest entry from the float64 statement — and so does the float32 evaluation of
    the statement (9.90e-5 from float64, 1.8e-5 from the reference's): the distance is float32's, not a difference of the
    two programs.  The fixture's batch is the first 96 triples of an unshuffled epoch, 10 distinct users, user 0 in 36 rows;
    SGL's InfoNCE takes the raw ids, so those 36 equal rows share the softmax's mass (36 terms of e^(1/T) each), and a row's
    gradient (sum_j p_ij n2_j - n2_i, projected off n1_i, with n1_i and n2_i nearly parallel) is what two cancellations leave
    of O(1) terms: float32 rounding arrives some 1e3 times amplified, all of it in d loss_users / d view (1.0e-4 of its own
    largest entry; BPR, the regulariser and the item term agree to 1.5e-6).  The bound is twice the measured figure."""
    e64, e32 = _anchor(golden_small, golden_next, operators, "SGL", "sgl")
    bound = max(2 * SGL_MEASURED, 1e-5)
    assert e64 <= bound and e32 <= bound


# ------------------------------------------------------------------------------------------------ no fragile entries
def _table(operators, graph, d):
    return ref.table(operators[graph][1], d, ref.table_seed(graph, d)).double()


@pytest.mark.parametrize("graph,K,inc,d", ref.MEAN_NOISE_CASES)
def test_no_fragile_entries_in_the_mean_noise_cases(operators, graph, K, inc, d):
    A, trace = operators[graph][0], []
    ref.propagate_noise64(A, _table(operators, graph, d), K, inc, ref.EPS, ref.NOISE_SEED, ref.SIDS[0], 1, trace=trace)
    assert len(trace) == K and ref.fragile_in(trace, A) == 0


@pytest.mark.parametrize("graph,K,inc,d,n_views", ref.VIEWS_CASES)
def test_no_fragile_entries_in_the_views_cases(operators, graph, K, inc, d, n_views):
    A, trace = operators[graph][0], []
    ref.views64(A, _table(operators, graph, d), K, inc, ref.EPS, ref.pass_streams(n_views), trace=trace)
    assert len(trace) == K * n_views and ref.fragile_in(trace, A) == 0


@pytest.mark.parametrize("graph,K,inc,d,n_views", ref.AUTOGRAD_CASES)
def test_no_fragile_entries_in_the_autograd_cases(operators, graph, K, inc, d, n_views):
    A, trace = operators[graph][0], []
    ref.views64(A, _table(operators, graph, d), K, inc, ref.EPS, ref.autograd_streams(n_views), trace=trace)
    assert len(trace) == K * n_views and ref.fragile_in(trace, A) == 0


def test_fragile_counts_what_it_should(operators):
    A = torch.tensor([[0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    X = torch.tensor([[1.0, 1.0, 0.0], [-1.0 + 1e-7, -1.0 + 1e-5, 0.0], [3.0, 3.0, 3.0]], dtype=torch.float64)
    # row 0: 0.5e-7 against a bound of 16 * 2^-24 * 1 = 9.5e-7 (fragile), 0.5e-5 (safe), an exact zero; row 1: no entries
    assert ref.fragile(A, X, A @ X) == 1


@pytest.mark.parametrize("name,layers", [r for r in ref.FUSED_RUNS if r[0] != "SGL"])  # (SGL draws no noise: nothing can flip)
def test_no_fragile_entries_along_the_fused_runs(golden_small, operators, name, layers):
    """Three steps of the float64 statement on graph_small's batches from the seed-2024 tables, the table rounded to float32
    before each step (what the GPU test reads back): no fragile entry in any layer of any perturbed pass."""
    g = golden_small
    A, n, U = operators["small"]
    cfg = ref.read_config(name, GCN_layer=layers)
    W0 = torch.from_numpy(np.concatenate([g["d64_init_user"], g["d64_init_item"]])).double()
    W, grads = W0, []
    for i, bt in enumerate(ref.fused_batches(g), 1):
        trace = []
        losses, dE = ref.engine_step64(name, [A], W.float(), U, bt, cfg, i, trace=trace)
        assert len(trace) == layers * (2 if name == "SimGCL" else 1) and ref.fragile_in(trace, A) == 0
        assert bool(torch.isfinite(losses).all())
        grads.append(dE)
        W = ref.adam64(W0, grads, lr=float(cfg["learn_rate"]))[-1][0]
    assert float((W - W0).abs().max()) > 1e-3  # three Adam steps moved the table
