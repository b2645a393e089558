"""MixRec, host side: the fixture regenerates from the reference and holds both settings; tests/mixrec_ref64.py — the float64
statement tests/test_gpu_mixrec.py holds the kernels against — fed the reference's RECORDED draws reproduces the reference's
loss list, both gradients and the rating, and its collapsed form equals the call-by-call composition; mixrec.draw_mix under
the generator's seeds returns the recorded draws exactly; the settings file carries every key the plugin reads; the plugin
resolves and refuses what it cannot run; header / binding / library agree on the entry points of csrc/idg_mixnce.hip, and
their argument checks come before any device work.

The fixture is the reference's own program run in float64 from its float32 initial tables (scripts/gen_golden_mixrec.py),
so the statement is held to it at rtol 1e-6 (losses) and 1e-6 of the largest entry (gradients).  Measured here: losses equal
to 3e-16, gradients 3.1e-8 (`def`) and 5.1e-8 (`mid`) of their largest entry — the float32 rounding of the stored arrays.
The float32 yardstick (the same composition in float32 against float64, on the fixture's inputs): losses 2.9e-7, gradients
5.5e-6 (`def`) and 5.4e-6 (`mid`) of their largest entry; tests/test_gpu_mixrec.py takes its gradient bound from it."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import mixrec_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mixrec_small.npz")
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="1000", early_stopping="10",
            interval="10", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.001", reg_lambda="0.0001",
            GCN_layer="3", ssl_lambda="1.1", temperature="0.2", alpha="0.1", beta="0.1", gamma="0.1", sparsity_test="0")
TAGS = ("def", "mid")
PARAMS = ("user_embedding", "item_embedding")
REG, SSL, TEMP, LAYERS = 1e-4, 1.1, 0.2, 2  # what the goldens were taken with


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "MixRec.txt"), "MixRec")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _draws(g, prefix):
    return (float(g[prefix + "_betas"][0]), float(g[prefix + "_betas"][1]), torch.from_numpy(g[prefix + "_nu"]),
            torch.from_numpy(g[prefix + "_user_perm"]), torch.from_numpy(g[prefix + "_item_perm"]))


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_mixrec.py")], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    assert open(FIXTURE, "rb").read() == open(str(tmp_path / "mixrec_small.npz"), "rb").read()


def test_fixture_holds_both_settings():
    assert os.path.getsize(FIXTURE) < (1 << 20)
    g = np.load(FIXTURE, allow_pickle=False)
    assert g["init_user_embedding"].shape == (300, 64) and g["init_item_embedding"].shape == (250, 64)
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    gs = np.load(os.path.join(ROOT, "tests", "golden", "graph_small.npz"), allow_pickle=False)
    cold = 300 + int(g["cold_item"][0])
    assert int(g["cold_item"][0]) in b[:, 2].tolist() and gs["adj_indptr"][cold + 1] == gs["adj_indptr"][cold]  # no training edge
    assert g["traj_batches"].shape == (768, 3) and g["rating_users"].shape == (32,)
    for tag in TAGS:
        for prefix, B in [(tag, 96)] + [("%s_traj%d" % (tag, i), 256) for i in range(3)]:
            betas = g[prefix + "_betas"]
            assert betas.shape == (2,) and ((betas > 0) & (betas < 1)).all()
            if tag == "mid":  # both halves of every term carry weight
                assert ((betas >= 0.2) & (betas <= 0.8)).all()
            nu = g[prefix + "_nu"]
            assert nu.dtype == np.float32 and nu.shape == (B,) and abs(float(nu.astype(np.float64).sum()) - 1) < 1e-5
            for side in ("user", "item"):
                assert sorted(g["%s_%s_perm" % (prefix, side)].tolist()) == list(range(B))
        assert g[tag + "_loss"].shape == (4,) and g[tag + "_traj_loss"].shape == (3, 4) and g[tag + "_rating"].shape == (32, 250)
        assert np.isfinite(g[tag + "_loss"]).all() and (g[tag + "_loss"] > 0).all()
        for p in PARAMS:
            for pre in ("grad", "traj"):
                a = g["%s_%s_%s" % (tag, pre, p)]
                assert a.shape == g["init_" + p].shape and a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
            moved = np.abs(g["%s_traj_%s" % (tag, p)] - g["init_" + p]).max()
            assert 1e-4 < moved <= 3.01e-3  # three Adam steps at lr = 1e-3


# ------------------------------------------------------------------------------- the float64 statement is the reference's
@pytest.mark.parametrize("tag", TAGS)
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, gs = np.load(FIXTURE, allow_pickle=False), golden_small
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (n, n))
    E0 = torch.from_numpy(np.concatenate([g["init_user_embedding"], g["init_item_embedding"]]))
    b = torch.from_numpy(g["batch"])
    draws = _draws(g, tag)
    losses, gE0, X = ref.step64(A, E0, b[:, 0], b[:, 1], b[:, 2], draws, LAYERS, REG, SSL, TEMP, U)
    assert losses.dtype == gE0.dtype == X.dtype == torch.float64 and losses.shape == (4,) and gE0.shape == (n, 64)
    want = np.concatenate([g[tag + "_grad_user_embedding"], g[tag + "_grad_item_embedding"]])
    e_loss = float(np.abs(losses.numpy() / g[tag + "_loss"] - 1).max())
    e_grad = float(np.abs(gE0.numpy() - want).max() / np.abs(want).max())
    print("%s: losses %.2e (relative), gradients %.2e of the largest entry from the fixture" % (tag, e_loss, e_grad))
    np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=1e-6)
    assert e_grad <= 1e-6
    assert float(X[U + int(g["cold_item"][0])].abs().max()) == 0  # the negative without a training edge: a zero row
    users = torch.from_numpy(g["rating_users"])
    np.testing.assert_allclose(torch.sigmoid(X[users] @ X[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-6, atol=1e-7)
    # the collapsed form is the call-by-call composition
    l_c, g_c, _ = ref.step64(A, E0, b[:, 0], b[:, 1], b[:, 2], draws, LAYERS, REG, SSL, TEMP, U, composed=True)
    assert float(((l_c - losses) / losses).abs().max()) <= 1e-13 and float((g_c - gE0).abs().max() / gE0.abs().max()) <= 1e-12
    # the same composition in float32: the yardstick the GPU file's gradient bound is taken from
    l32, g32, _ = ref.step64(A, E0, b[:, 0], b[:, 1], b[:, 2], draws, LAYERS, REG, SSL, TEMP, U, dtype=torch.float32, composed=True)
    e32 = float((g32.double() - gE0).abs().max() / gE0.abs().max())
    print("%s: the float32 composition: losses %.2e, gradients %.2e of the largest entry from float64"
          % (tag, float(((l32.double() - losses) / losses).abs().max()), e32))
    assert e32 < 1e-4


def test_collapsed_side_equals_composition_on_edge_cases():
    """Fixed points, the identity, beta at both ends, a one-hot nu and a zero row: loss and gradient in float64."""
    gen = torch.Generator().manual_seed(5)
    B, d = 37, 24
    x0 = torch.randn(B, d, dtype=torch.float64, generator=gen)
    x0[4] = 0
    perm = torch.randperm(B, generator=gen)
    j = perm.tolist().index(3)
    perm[j], perm[3] = perm[3].item(), 3  # a fixed point; still a permutation
    assert sorted(perm.tolist()) == list(range(B)) and int(perm[3]) == 3
    one_hot = torch.zeros(B)
    one_hot[11] = 1
    for pi in (perm, torch.arange(B)):
        for beta in (0.0, 1.0, 1e-6, 0.37):
            for nu in (torch.rand(B, generator=gen), one_hot):
                a, c = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
                la, lc = ref.side64(a, pi, beta, nu.double(), 0.2), ref.side_composed(c, pi, beta, nu.double(), 0.2)
                (ga,), (gc,) = torch.autograd.grad(la, a), torch.autograd.grad(lc, c)
                live = torch.arange(B) != 4  # (the zero row's gradient carries normalize's 1e12: compared on its own scale)
                assert abs(float(la.detach() - lc.detach())) <= 1e-13 * abs(float(lc.detach()))
                assert float((ga[live] - gc[live]).abs().max()) <= 1e-12 * float(gc[live].abs().max())
                assert float((ga[4] - gc[4]).abs().max()) <= 1e-12 * max(float(gc[4].abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------------------ the draws
def test_draw_mix_returns_the_recorded_draws():
    from idgrec_amd.mixrec import draw_mix

    g = np.load(FIXTURE, allow_pickle=False)
    seeds = g["draw_seeds"].tolist()
    state_np, state_t = np.random.get_state(), torch.get_rng_state()
    try:
        for tag in TAGS:
            alpha, beta, gamma = g[tag + "_abg"].tolist()
            for seed, (prefix, B) in zip(seeds, [(tag, 96)] + [("%s_traj%d" % (tag, i), 256) for i in range(3)]):
                np.random.seed(seed)
                torch.manual_seed(seed)
                ub, ib, nu, up, ip = draw_mix(B, alpha, beta, gamma)
                assert isinstance(ub, float) and isinstance(ib, float)
                assert [ub, ib] == g[prefix + "_betas"].tolist()
                assert nu.dtype == torch.float32 and nu.shape == (B,) and np.array_equal(nu.numpy(), g[prefix + "_nu"])
                assert up.dtype == ip.dtype == torch.int64
                assert np.array_equal(up.numpy(), g[prefix + "_user_perm"]) and np.array_equal(ip.numpy(), g[prefix + "_item_perm"])
    finally:
        np.random.set_state(state_np)
        torch.set_rng_state(state_t)


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_has_every_key_the_plugin_reads():
    cfg = _cfg()
    assert dict(cfg) == KEYS and list(dict(cfg)) == list(KEYS)
    src = open(os.path.join(ROOT, "models", "MixRec.py")).read() + open(os.path.join(ROOT, "id-grec_amd", "modeling.py")).read()
    read = set(re.findall(r"config\[['\"](\w+)['\"]\]", src))
    assert {"embedding_size", "GCN_layer", "reg_lambda", "ssl_lambda", "temperature", "alpha", "beta", "gamma"} <= read
    assert read <= set(KEYS), read - set(KEYS)
    import utility.utility_function.tools as tools

    common = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    assert set(common) <= set(KEYS)  # the common keys of configure/LightGCN.txt are all there


def test_plugin_resolves_and_refuses_what_it_cannot_run(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    mod = importlib.import_module("models.MixRec")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.MixRec
    assert cls.supports_fused_step and cls.n_fused_losses == 4 and cls.include_layer0 is False and cls.mix_source is None
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels"):
        assert callable(getattr(cls, name)), name
    assert not hasattr(cls, "mix_aggregate")  # dead code in the reference
    from idgrec_amd.modeling import EngineStep, PackedRecommender

    assert issubclass(cls, PackedRecommender) and issubclass(cls, EngineStep)
    assert cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="MixRec needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))


def test_main_names_mixrec_as_implemented():
    main = open(os.path.join(ROOT, "main.py")).read()
    assert "MixRec" in re.split(r"[,.\s]+", main.split("Implemented:")[1].split("\n")[0])
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "MixRec" in [ln for ln in readme.split("\n") if "python main.py --model=" in ln][0]


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_mix_nce_workspace_bytes", 2), ("idg_mix_nce_f32", 20))


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
    assert '"idg_mixnce.hip"' in build.split("SOURCES")[1].split("]")[0]
    L = native.lib
    assert 0 < L.idg_mix_nce_workspace_bytes(2048, 64) < (64 << 20) and L.idg_mix_nce_workspace_bytes(2048, 64) % 256 == 0
    assert 0 < L.idg_mix_nce_workspace_bytes(1, 1) and 0 < L.idg_mix_nce_workspace_bytes(257, 256)
    for B, d in ((0, 64), (-1, 64), (96, 0), (96, 257), (1 << 22, 64)):
        assert L.idg_mix_nce_workspace_bytes(B, d) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry point can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    P0, U0, I0, N0, UP0, IP0, NU0, L0, G0, WS0 = tuple(0x100000 * i for i in range(1, 10)) + (0x4000000,)

    def call(panel=P0, n=550, d=64, U=300, users=U0, pos=I0, neg=N0, B=96, up=UP0, ip=IP0, nu=NU0, ub=0.5, ib=0.5, t=0.2, w=1.1,
             loss=L0, g=G0, ws=WS0):
        return L.idg_mix_nce_f32(panel, n, d, U, users, pos, neg, B, up, ip, nu, ub, ib, t, w, loss, None, g, ws, None)

    cases = ((dict(panel=None), "NULL"), (dict(users=None), "NULL"), (dict(pos=None), "NULL"), (dict(neg=None), "NULL"),
             (dict(up=None), "NULL"), (dict(ip=None), "NULL"), (dict(nu=None), "NULL"), (dict(ws=None), "NULL"),
             (dict(B=0), "B = 0"), (dict(B=1 << 22), "B ="), (dict(d=0), "d = 0"), (dict(d=257), "d = 257"),
             (dict(U=0), "bad panel"), (dict(U=550), "bad panel"), (dict(t=0.0), "temperature"), (dict(t=-1.0), "temperature"),
             (dict(t=float("nan")), "temperature"), (dict(ub=-0.1), "mixing weights"), (dict(ib=1.5), "mixing weights"),
             (dict(ub=float("nan")), "mixing weights"), (dict(w=float("inf")), "ssl_weight"), (dict(loss=None, g=None), "nothing to compute"),
             (dict(panel=P0 + 2), "misaligned"), (dict(g=G0 + 1), "misaligned"), (dict(nu=NU0 + 2), "misaligned"),
             (dict(loss=L0 + 2), "misaligned"), (dict(ws=WS0 + 128), "misaligned"), (dict(g=P0), "overlaps"),
             (dict(g=P0 + 550 * 64 * 4 - 4), "overlaps"))
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_mix_nce_f32" in msg and word in msg, (kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    X = torch.zeros(10, 64)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.mix_nce(X, 5, ids, ids, ids, ids, ids, torch.zeros(4), 0.5, 0.5, 0.2, 1.0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.mix_nce_raw(X, 5, ids, ids, ids, ids, ids, torch.zeros(4), 0.5, 0.5, 0.2, 1.0)
    with pytest.raises(ValueError, match="not built"):
        ops.mix_nce_workspace(96, 300, "cpu")
