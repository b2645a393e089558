"""LightGCL, host side: the fixture regenerates from the reference and holds both settings; tests/lightgcl_ref64.py — the
float64 statement tests/test_gpu_lightgcl.py holds the kernels against, written in the COLLAPSED form the kernels implement —
reproduces the reference's own float64 run (losses, both gradients, three Adam steps, the rating) in both settings, which
proves the collapse identity and the clamp handling against the reference itself; its log-sum-exp is finite and exact where
exp overflows; the symmetric adjacency's user-row block is the reference's rectangular matrix; the settings file carries
every key the plugin reads; the plugin resolves and refuses what it cannot run; header / binding / library agree on the entry
points of csrc/idg_svdnce.hip, and their argument checks come before any device work.

Both sides of the pin are float64 (scripts/gen_golden_lightgcl.py stores the losses and gradients unrounded), so it is held at
1e-10 relative for the losses and 1e-10 of the largest entry for the gradients.  Measured here: losses 1.3e-15 (`def`) and
1.1e-15 (`clamp`), gradients 3.2e-16 and 3.1e-16 of their largest entry.  The float32 yardstick (the reference's layer-by-layer
expressions in float32 against the float64 statement, on the fixture's inputs; printed by the same test): losses 5.3e-8 and
2.8e-7, gradients 1.6e-7 and 2.3e-7 of the largest entry."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import lightgcl_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lightgcl_small.npz")
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="1000", early_stopping="10",
            interval="10", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.001", reg_lambda="1e-6",
            GCN_layer="2", ssl_lambda="0.5", temperature="0.2", svd_q="5", sparsity_test="0")
TAGS = ("def", "clamp")
PARAMS = ("user_embedding", "item_embedding")


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCL.txt"), "LightGCL")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def load(tag, gs):
    """(A, E0, svd_u, s, svd_v, hyper dict, U) of a setting, in float64."""
    g = np.load(FIXTURE, allow_pickle=False)
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.symmetric_operator(g["R_indptr"], g["R_indices"], g["R_data"], U, n - U)  # the reference model's own values
    E0 = torch.from_numpy(np.concatenate([g[tag + "_init_user_embedding"], g[tag + "_init_item_embedding"]])).double()
    f = [torch.from_numpy(g[tag + k]).double() for k in ("_svd_u", "_s", "_svd_v")]
    reg, ssl, tau, K, q, lr = g[tag + "_hyper"].tolist()
    return g, A, E0, f, dict(reg=reg, ssl=ssl, tau=tau, K=int(K), q=int(q), lr=lr), U


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_lightgcl.py")], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    assert open(FIXTURE, "rb").read() == open(str(tmp_path / "lightgcl_small.npz"), "rb").read()


def test_fixture_holds_both_settings():
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "mixrec_small.npz"))
    g = np.load(FIXTURE, allow_pickle=False)
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert len(set(b[:, 0].tolist())) > 48  # the users are mixed: not the sampler's user-by-user rows
    assert g["traj_batches"].shape == (384, 3) and g["rating_users"].shape == (32,)
    for tag, K, q in (("def", 2, 5), ("clamp", 3, 3)):
        assert g[tag + "_hyper"].tolist() == [1e-6, 0.5, 0.2, K, q, 1e-3]
        assert g[tag + "_svd_u"].shape == (300, q) and g[tag + "_s"].shape == (q,) and g[tag + "_svd_v"].shape == (250, q)
        assert g[tag + "_svd_u"].dtype == np.float32 and (np.diff(g[tag + "_s"]) <= 0).all() and (g[tag + "_s"] > 0).all()
        assert g[tag + "_loss"].shape == (3,) and g[tag + "_traj_loss"].shape == (3, 3) and g[tag + "_rating"].shape == (32, 250)
        assert np.isfinite(g[tag + "_loss"]).all() and g[tag + "_loss"].dtype == np.float64
        for p, rows in zip(PARAMS, (300, 250)):
            assert g["%s_init_%s" % (tag, p)].shape == (rows, 32) and g["%s_init_%s" % (tag, p)].dtype == np.float32
            a = g["%s_grad_%s" % (tag, p)]
            assert a.shape == (rows, 32) and a.dtype == np.float64 and np.isfinite(a).all() and np.abs(a).max() > 0
            moved = np.abs(g["%s_traj_%s" % (tag, p)] - g["%s_init_%s" % (tag, p)]).max()
            assert 1e-4 < moved <= 3.01e-3  # three Adam steps at lr = 1e-3
        for side in ("_pos_u", "_pos_i"):
            pos = g[tag + side]
            assert pos.shape == (96,)
            if tag == "clamp":  # the clamp is active on a real share of the rows, and no row sits at the kink
                assert 0.2 <= float((np.abs(pos) > 5).mean()) <= 0.8 and float(np.abs(np.abs(pos) - 5).min()) > 1e-3
            else:
                assert float(np.abs(pos).max()) < 5
    scale = float(g["clamp_scale"][0])
    np.testing.assert_allclose(g["clamp_init_user_embedding"], g["def_init_user_embedding"] * np.float32(scale), rtol=1e-6)


# ------------------------------------------------------------------------------- the float64 statement is the reference's
@pytest.mark.parametrize("tag", TAGS)
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, A, E0, (su, s, sv), h, U = load(tag, golden_small)
    b = torch.from_numpy(g["batch"])
    losses, grad, F, parts = ref.step64(A, E0, su, s, sv, b[:, 0], b[:, 1], b[:, 2], h["K"], h["reg"], h["ssl"], h["tau"], U)
    assert losses.dtype == grad.dtype == torch.float64 and losses.shape == (3,) and grad.shape == E0.shape
    want = np.concatenate([g[tag + "_grad_user_embedding"], g[tag + "_grad_item_embedding"]])
    e_loss = float(np.abs(losses.numpy() / g[tag + "_loss"] - 1).max())
    e_grad = float(np.abs(grad.numpy() - want).max() / np.abs(want).max())
    print("%s: losses %.2e (relative), gradients %.2e of the largest entry from the fixture" % (tag, e_loss, e_grad))
    assert e_loss <= 1e-10 and e_grad <= 1e-10
    # the unclamped positives, row by row: which rows clamp is the reference's
    _, g_u, g_i = ref.views_collapsed(A, E0, su, s, sv, h["K"], U, b[:, 0], b[:, 1])
    np.testing.assert_allclose(ref.positives(g_u, F[:U], b[:, 0], h["tau"]).numpy(), g[tag + "_pos_u"], rtol=1e-10)
    np.testing.assert_allclose(ref.positives(g_i, F[U:], b[:, 1], h["tau"]).numpy(), g[tag + "_pos_i"], rtol=1e-10)
    users = torch.from_numpy(g["rating_users"])
    np.testing.assert_allclose(torch.sigmoid(F[users] @ F[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-6, atol=1e-7)
    # the layered form (the reference's expressions) equals the collapsed one
    l_l, g_l, _, _ = ref.step64(A, E0, su, s, sv, b[:, 0], b[:, 1], b[:, 2], h["K"], h["reg"], h["ssl"], h["tau"], U, layered=True)
    assert float(((l_l - losses) / losses).abs().max()) <= 1e-12 and float((g_l - grad).abs().max() / grad.abs().max()) <= 1e-12
    # the same layered composition in float32: the yardstick of the GPU file's bounds
    l32, g32, _, _ = ref.step64(A, E0, su, s, sv, b[:, 0], b[:, 1], b[:, 2], h["K"], h["reg"], h["ssl"], h["tau"], U,
                                dtype=torch.float32, layered=True)
    e32 = float((g32.double() - grad).abs().max() / grad.abs().max())
    print("%s: the float32 composition: losses %.2e, gradients %.2e of the largest entry from float64"
          % (tag, float(((l32.double() - losses) / losses).abs().max()), e32))
    assert e32 < 1e-4


@pytest.mark.parametrize("tag", TAGS)
def test_float64_statement_reproduces_three_adam_steps(tag, golden_small):
    g, A, E0, (su, s, sv), h, U = load(tag, golden_small)
    batches = [torch.from_numpy(g["traj_batches"][i * 128:(i + 1) * 128]) for i in range(3)]
    losses, panels = ref.adam_steps(A, E0, su, s, sv, batches, h["K"], h["reg"], h["ssl"], h["tau"], U, h["lr"])
    np.testing.assert_allclose(losses.numpy(), g[tag + "_traj_loss"], rtol=1e-10)
    want = np.concatenate([g[tag + "_traj_user_embedding"], g[tag + "_traj_item_embedding"]])
    assert float(np.abs(panels[-1].numpy() - want).max()) <= 1e-7 * float(np.abs(want).max())  # stored rounded to float32


def test_clamped_rows_carry_no_positive_gradient(golden_small):
    """In the `clamp` setting the positive term's gradient w.r.t. a view row is exactly zero where the row clamps."""
    g, A, E0, (su, s, sv), h, U = load("clamp", golden_small)
    b = torch.from_numpy(g["batch"])
    F, EK = ref.propagate(A, E0, h["K"])
    P_i = sv.t() @ (F - EK)[U:]
    _, gF, gE, dP, pos, _ = ref.svd_nce64(F, E0, 0, U, su * s, P_i, b[:, 0], h["tau"], upstream=(0.0, 1.0))
    clamped = pos.abs() > 5
    assert 0 < int(clamped.sum()) < pos.numel()
    only_clamped = torch.ones(U, dtype=torch.bool)
    only_clamped[b[:, 0][~clamped]] = False  # users none of whose occurrences is inside the clamp
    assert float(gE[:U][only_clamped].abs().max()) == 0 and float(gF[:U][only_clamped].abs().max()) == 0
    assert float(gE[:U][b[:, 0][~clamped]].abs().min(dim=1).values.max()) > 0


def test_log_sum_exp_is_finite_and_exact_where_exp_overflows():
    gen = torch.Generator().manual_seed(3)
    s = torch.randn(7, 50, dtype=torch.float64, generator=gen) * 30
    s[0, 3], s[1, :] = 200.0, -200.0
    s[2] = s[2] - 1000
    got = ref.lse_guarded(s)
    assert torch.isfinite(got).all()
    want = torch.logsumexp(torch.cat([s, torch.full((7, 1), float(np.log(1e-8)), dtype=torch.float64)], 1), dim=1)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-13)
    assert abs(float(got[0]) - 200.0) < 1e-6 and abs(float(got[1]) - float(np.log(1e-8))) < 1e-9
    # in float32 the reference's expression overflows there; the statement's does not
    s32 = s.float()
    assert not torch.isfinite(torch.log(torch.exp(s32).sum(1) + 1e-8)).all()
    got32 = ref.lse_guarded(s32)
    assert torch.isfinite(got32).all() and float((got32.double() - want).abs().max()) < 1e-4 * 200


# ------------------------------------------------------------------------------------------------------------ the graph
@pytest.mark.parametrize("gname", ["tiny", "small"])
def test_user_row_block_of_the_symmetric_adjacency_is_the_rectangular_matrix(gname, tmp_path, golden_tiny, golden_small):
    import utility.utility_data.data_graph as data_graph
    import utility.utility_data.data_loader as data_loader

    g = golden_tiny if gname == "tiny" else golden_small
    d = tmp_path / gname
    d.mkdir()
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    data = data_loader.Data(str(d), dict(dataset=gname, dataset_path=str(tmp_path) + "/", sparsity_test="0"))
    U, I = data.num_users, data.num_items
    A = data_graph.sparse_adjacency_matrix(data)
    R = data_graph.sparse_adjacency_matrix_R(data)
    block, blockT = A[:U, U:].tocsr(), A[U:, :U].tocsr()
    assert block.shape == R.shape == (U, I) and block.nnz == R.nnz
    assert A[:U, :U].nnz == 0 and A[U:, U:].nnz == 0
    diff = abs(block.astype(np.float64) - R.astype(np.float64))
    assert diff.max() <= 2 * np.finfo(np.float32).eps * abs(R).max()  # float32 rounding of one product of two roots
    assert abs(blockT - block.T).max() == 0


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_has_every_key_the_plugin_reads():
    cfg = _cfg()
    assert dict(cfg) == KEYS and list(dict(cfg)) == list(KEYS)
    src = open(os.path.join(ROOT, "models", "LightGCL.py")).read() + open(os.path.join(ROOT, "id-grec_amd", "modeling.py")).read()
    read = set(re.findall(r"config\[['\"](\w+)['\"]\]", src))
    assert {"embedding_size", "GCN_layer", "reg_lambda", "ssl_lambda", "temperature", "svd_q"} <= read
    assert read <= set(KEYS), read - set(KEYS)
    import utility.utility_function.tools as tools

    common = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    assert set(common) <= set(KEYS)  # the common keys of configure/LightGCN.txt are all there


def test_plugin_resolves_and_refuses_what_it_cannot_run(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    mod = importlib.import_module("models.LightGCL")
    assert callable(mod.Trainer) and callable(mod.Trainer.train) and callable(mod.svd_factors)
    cls = mod.LightGCL
    assert cls.supports_fused_step and cls.n_fused_losses == 3 and cls.include_layer0 is True and cls.factor_source is None
    assert cls.FUSED_WIDTHS == (32, 64, 128, 256)
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels", "set_factors", "lightgcl_engine"):
        assert callable(getattr(cls, name)), name
    assert not hasattr(cls, "sparse_dropout")  # commented out of the reference's aggregate()
    from idgrec_amd.modeling import EngineStep, PackedRecommender

    assert issubclass(cls, PackedRecommender) and issubclass(cls, EngineStep)
    assert cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="LightGCL needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))
    for q in ("0", "17"):
        with pytest.raises(ValueError, match="svd_q"):
            cls(dict(cfg, svd_q=q), data, torch.device("cpu"))
    with pytest.raises(ValueError, match="temperature"):
        cls(dict(cfg, temperature="0"), data, torch.device("cpu"))
    with pytest.raises(KeyError):
        cls({k: v for k, v in cfg.items() if k != "svd_q"}, data, torch.device("cpu"))


def test_svd_factors_on_the_host_are_a_truncated_svd(tmp_path, golden_small):
    """The plugin's factor helper on the CPU: orthonormal columns and descending singular values that are Ritz values of the
    matrix — never above the exact ones, the leading one close (the spectrum of `small` is flat below it, and a randomised
    range of q columns with two power iterations, which is what the reference takes, captures the rest only in part)."""
    import scipy.sparse as sp

    from models.LightGCL import svd_factors

    gs = golden_small
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = sp.csr_matrix((gs["adj_data"], gs["adj_indices"], gs["adj_indptr"]), shape=(n, n))
    R = A[:U, U:]
    state = torch.get_rng_state()
    try:
        torch.manual_seed(0)
        su, s, sv = svd_factors(R, 5, torch.device("cpu"))
    finally:
        torch.set_rng_state(state)
    assert su.shape == (U, 5) and s.shape == (5,) and sv.shape == (n - U, 5) and su.dtype == torch.float32
    assert float((su.t() @ su - torch.eye(5)).abs().max()) < 1e-4 and float((sv.t() @ sv - torch.eye(5)).abs().max()) < 1e-4
    exact = np.linalg.svd(R.toarray().astype(np.float64), compute_uv=False)[:5]
    assert (np.diff(s.numpy()) <= 0).all() and (s.numpy() <= exact * (1 + 1e-4)).all() and abs(s.numpy()[0] / exact[0] - 1) < 0.05
    approx = (su * s) @ sv.t()
    assert float((su.t() @ torch.from_numpy(R.toarray()) @ sv - torch.diag(s)).abs().max()) < 1e-4  # S = U^T R V
    assert approx.shape == (U, n - U)


def test_main_names_lightgcl_as_implemented():
    main = open(os.path.join(ROOT, "main.py")).read()
    assert "LightGCL" in re.split(r"[,.\s]+", main.split("Implemented:")[1].split("\n")[0])
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "LightGCL" in [ln for ln in readme.split("\n") if "python main.py --model=" in ln][0]


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_lowrank_project_workspace_bytes", 3), ("idg_lowrank_project_f32", 12), ("idg_lowrank_expand_f32", 12),
                ("idg_svd_nce_workspace_bytes", 4), ("idg_svd_nce_f32", 18))


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1))
    for name, n_args in ENTRY_POINTS:
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(native.PROTOTYPES[name][1]), name
        assert hasattr(native.lib, name)
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_svdnce.hip"' in build.split("SOURCES")[1].split("]")[0]
    L = native.lib
    ws = L.idg_svd_nce_workspace_bytes(2048, 38048, 64, 5)
    assert 0 < ws < (256 << 20) and ws % 256 == 0
    assert 0 < L.idg_svd_nce_workspace_bytes(1, 1, 1, 1) and 0 < L.idg_svd_nce_workspace_bytes(300, 1000, 256, 16)
    for B, N, d, q in ((0, 10, 64, 5), (10, 0, 64, 5), (10, 10, 0, 5), (10, 10, 257, 5), (10, 10, 64, 0), (10, 10, 64, 17),
                       (10, 1 << 31, 64, 5)):
        assert L.idg_svd_nce_workspace_bytes(B, N, d, q) == 0
    assert 0 < L.idg_lowrank_project_workspace_bytes(1, 1, 1) <= L.idg_lowrank_project_workspace_bytes(30000000, 16, 256)
    assert L.idg_lowrank_project_workspace_bytes(30000000, 16, 256) <= 1024 * 16 * 256 * 4 + 256  # at most 1024 partials
    for n, q, d in ((0, 5, 64), (10, 0, 64), (10, 17, 64), (10, 5, 0), (10, 5, 257)):
        assert L.idg_lowrank_project_workspace_bytes(n, q, d) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    F0, E0, AS0, P0, ID0, L0, GF0, GE0, DP0, WS0 = tuple(0x100000 * i for i in range(1, 10)) + (0x4000000,)

    def nce(F=F0, E=E0, row0=0, N=300, d=64, AS=AS0, q=5, P=P0, ids=ID0, B=96, t=0.2, loss=L0, gF=GF0, gE=GE0, dP=DP0, ws=WS0):
        return L.idg_svd_nce_f32(F, E, row0, N, d, AS, q, P, ids, B, t, loss, None, gF, gE, dP, ws, None)

    cases = ((dict(F=None), "NULL"), (dict(E=None), "NULL"), (dict(AS=None), "NULL"), (dict(P=None), "NULL"), (dict(ids=None), "NULL"),
             (dict(ws=None), "NULL"), (dict(B=0), "B = 0"), (dict(N=0), "N = 0"), (dict(row0=-1), "row0 = -1"), (dict(d=0), "d = 0"),
             (dict(d=257), "d = 257"), (dict(q=0), "q = 0"), (dict(q=17), "q = 17"), (dict(N=1 << 31), "int32"),
             (dict(t=0.0), "temperature"), (dict(t=-1.0), "temperature"), (dict(t=float("nan")), "temperature"),
             (dict(gE=None), "go together"), (dict(dP=None), "go together"), (dict(gF=None), "go together"),
             (dict(loss=None, gF=None, gE=None, dP=None), "nothing to compute"), (dict(ws=WS0 + 128), "256-byte"))
    for kw, word in cases:
        assert nce(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_svd_nce_f32" in msg and word in msg, (kw, msg)

    def proj(A=AS0, lda=5, X=F0, ldx=64, n=100, q=5, d=64, out=P0, ws=WS0):
        return L.idg_lowrank_project_f32(A, lda, None, X, ldx, n, q, d, out, 0, ws, None)

    for kw, word in ((dict(A=None), "NULL"), (dict(X=None), "NULL"), (dict(out=None), "NULL"), (dict(ws=None), "NULL"),
                     (dict(n=0), "n = 0"), (dict(q=17), "q = 17"), (dict(d=257), "d = 257"), (dict(lda=4), "leading dimension"),
                     (dict(ldx=63), "leading dimension"), (dict(ws=WS0 + 4), "256-byte")):
        assert proj(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_lowrank_project_f32" in msg and word in msg, (kw, msg)

    def expand(A=AS0, lda=5, P=P0, n=100, q=5, d=64, Y=F0, ldy=64):
        return L.idg_lowrank_expand_f32(A, lda, None, P, n, q, d, 1.0, 0, Y, ldy, None)

    for kw, word in ((dict(A=None), "NULL"), (dict(P=None), "NULL"), (dict(Y=None), "NULL"), (dict(n=0), "n = 0"),
                     (dict(q=0), "q = 0"), (dict(d=300), "d = 300"), (dict(lda=4), "leading dimension"),
                     (dict(ldy=32), "leading dimension")):
        assert expand(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_lowrank_expand_f32" in msg and word in msg, (kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    F = torch.zeros(10, 64)
    ids = torch.zeros(4, dtype=torch.int64)
    AS, P = torch.zeros(5, 3), torch.zeros(3, 64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.svd_nce_loss(F, F, 0, 5, AS, P, ids, 0.2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.svd_nce_raw(F, F, 0, 5, AS, P, ids, 0.2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.lowrank_project(AS, torch.zeros(5, 64))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.lowrank_expand(AS, P)
    for kw, word in ((dict(N=11), "not inside"), (dict(AS=torch.zeros(4, 3)), "factor rows"), (dict(P=torch.zeros(2, 64)), "P is"),
                     (dict(t=0.0), "temperature"), (dict(ids=ids[:0]), "empty batch"), (dict(AS=torch.zeros(5, 17)), "factor rows")):
        a = dict(N=5, AS=AS, P=P, t=0.2, ids=ids)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.svd_nce_loss(F, F, 0, a["N"], a["AS"], a["P"], a["ids"], a["t"])
    with pytest.raises(ValueError, match="go together"):
        ops.svd_nce_raw(F, F, 0, 5, AS, P, ids, 0.2, g_final=torch.zeros_like(F))
    with pytest.raises(ValueError, match="not built"):
        ops.svd_nce_workspace(96, 300, 300, 5, "cpu")
