"""BIGCF, host side: the fixtures regenerate from the reference and hold both settings; tests/bigcf_ref64.py — the float64
statement tests/test_gpu_bigcf.py holds the kernels against — fed the reference's RECORDED noise reproduces the reference's
loss lists, every gradient and the rating, and its closed-form layer gradients equal float64 autograd; the settings file
carries every key the plugin reads; the plugin resolves and refuses what it cannot run; header / binding / library agree on
the entry points of csrc/idg_intent.hip; every argument check of theirs comes before any device work; the wrapper's errors."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import bigcf_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"def": os.path.join(ROOT, "tests", "golden", "bigcf_small.npz"), "one": os.path.join(ROOT, "tests", "golden", "bigcf_small_one.npz")}
# where the reference tree lives is stated once, by the golden generators (oracle/gen_golden.py)
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="1000", early_stopping="10",
            interval="10", embedding_size="64", intent_size="128", batch_size="2048", test_batch_size="2048", learn_rate="0.001",
            reg_lambda="0.0001", ssl_lambda="0.2", ssl_temperature="0.2", int_temperature="1.0", GCN_layer="2", sparsity_test="0")
LAYERS = {"def": 2, "one": 1}
PARAMS = ("user_embedding", "item_embedding", "user_intent", "item_intent")
RTOL = 1e-4  # tests/test_gccf_host.py
REG, SSL, TEMP = 1e-4, 0.2, 0.2  # configure/BIGCF.txt, what the goldens were taken with


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "BIGCF.txt"), "BIGCF")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _golden(tag):
    g = dict(np.load(FIXTURES["def"], allow_pickle=False))
    if tag != "def":
        g.update(np.load(FIXTURES[tag], allow_pickle=False))
    return g


# ------------------------------------------------------------------------------------------------------------ the fixtures
def test_fixtures_regenerate_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_bigcf.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    for path in FIXTURES.values():
        a, b = np.load(path, allow_pickle=False), np.load(str(tmp_path / os.path.basename(path)), allow_pickle=False)
        assert sorted(a.keys()) == sorted(b.keys())
        for k in a.keys():  # every array byte for byte
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        assert open(path, "rb").read() == open(str(tmp_path / os.path.basename(path)), "rb").read()


def test_fixtures_hold_both_settings():
    for path in FIXTURES.values():
        assert os.path.getsize(path) < (1 << 20)
    shared = np.load(FIXTURES["def"])
    assert shared["init_user_embedding"].shape == (300, 64) and shared["init_item_embedding"].shape == (250, 64)
    assert shared["init_user_intent"].shape == shared["init_item_intent"].shape == (64, 128)
    for name in ("noise_a", "noise_b"):
        z = shared[name]
        assert z.shape == (550, 64) and z.dtype == np.float32 and abs(float(z.mean())) < 0.03 and abs(float(z.var()) - 1) < 0.05
    assert not np.array_equal(shared["noise_a"], shared["noise_b"])
    b = shared["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert shared["traj_batches"].shape == (768, 3) and shared["rating_users"].shape == (32,)
    for tag in LAYERS:
        g = _golden(tag)
        assert g[tag + "_loss"].shape == (3,) and g[tag + "_traj_loss"].shape == (3, 3) and g[tag + "_rating"].shape == (32, 250)
        assert np.isfinite(g[tag + "_loss"]).all() and (g[tag + "_loss"] > 0).all()
        for p in PARAMS:
            for pre in ("grad", "traj"):
                a = g["%s_%s_%s" % (tag, pre, p)]
                assert a.shape == g["init_" + p].shape and a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
            moved = np.abs(g["%s_traj_%s" % (tag, p)] - g["init_" + p]).max()
            assert 1e-4 < moved <= 3.01e-3  # three Adam steps at lr = 1e-3


# ------------------------------------------------------------------------------- the float64 statement is the reference's
def _setting(golden_small, tag):
    g, gs = _golden(tag), golden_small
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (n, n))
    E0 = torch.from_numpy(np.concatenate([g["init_user_embedding"], g["init_item_embedding"]]))
    return g, U, A, E0, torch.from_numpy(g["init_user_intent"]), torch.from_numpy(g["init_item_intent"])


@pytest.mark.parametrize("tag", sorted(LAYERS))
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, U, A, E0, Wu, Wi = _setting(golden_small, tag)
    b = torch.from_numpy(g["batch"])
    Z = torch.from_numpy(g["noise_a"])
    losses, terms, (gE0, gWu, gWi), F, T = ref.step64(A, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], Z, LAYERS[tag], REG, SSL, TEMP, U)
    assert losses.dtype == gE0.dtype == F.dtype == torch.float64 and F.shape == T.shape == (550, 64) and terms.shape == (5,)
    np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=RTOL)
    np.testing.assert_allclose(gE0[:U].numpy(), g[tag + "_grad_user_embedding"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(gE0[U:].numpy(), g[tag + "_grad_item_embedding"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(gWu.numpy(), g[tag + "_grad_user_intent"], rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(gWi.numpy(), g[tag + "_grad_item_intent"], rtol=1e-3, atol=1e-7)
    # the reference's rating drew the second recorded panel
    users = torch.from_numpy(g["rating_users"])
    Fb = ref.step64(A, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], torch.from_numpy(g["noise_b"]), LAYERS[tag], REG, SSL, TEMP, U)[3]
    np.testing.assert_allclose(torch.sigmoid(Fb[users] @ Fb[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    # the same expressions in float32: the yardstick the GPU file measures the kernels with
    l32, _, g32, F32_, _ = ref.step64(A, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], Z, LAYERS[tag], REG, SSL, TEMP, U, dtype=torch.float32)
    assert l32.dtype == g32[0].dtype == F32_.dtype == torch.float32
    for name, a, x, y in (("d E0", np.concatenate([g[tag + "_grad_user_embedding"], g[tag + "_grad_item_embedding"]]), gE0, g32[0]),
                          ("d W_u", g[tag + "_grad_user_intent"], gWu, g32[1]), ("d W_i", g[tag + "_grad_item_intent"], gWi, g32[2])):
        e_ref, e_f32 = ref.errors(a, x, y)
        print("%s %s: the reference %.2e, the float32 composition %.2e of max from float64" % (tag, name, e_ref, e_f32))
        assert e_f32 < 1e-3  # (a float32 run sits as far from float64 as the reference's own float32 numbers are allowed above)


@pytest.mark.parametrize("case", ["all rows", "two rows, NaN elsewhere", "gT absent", "gT at some of the rows", "a zero row"])
def test_closed_form_layer_gradients_equal_float64_autograd(case):
    gen = torch.Generator().manual_seed(11)
    n, d, k = 50, 64, 128
    X, W, Z, gF, gT = (torch.randn(s, dtype=torch.float64, generator=gen) * a for s, a in
                       (((n, d), 0.3), ((d, k), 0.4), ((n, d), 1.0), ((n, d), 1.0), ((n, d), 1.0)))
    rows, gt = None, gT
    nan = torch.full_like(X, float("nan"))
    keep = torch.ones(n, dtype=torch.bool)
    if case == "two rows, NaN elsewhere":
        rows = [0, n - 1]
        keep = ref._flags(rows, n, "cpu")
    elif case == "gT absent":
        gt = None
    elif case == "gT at some of the rows":
        gt = torch.where((torch.arange(n) % 2 == 0)[:, None], gT, torch.zeros_like(gT))
    elif case == "a zero row":
        X[7] = 0
    x, w = X.clone().requires_grad_(True), W.clone().requires_grad_(True)
    F, T = ref.intent64(x, w, Z)
    if case == "a zero row":
        assert float((torch.softmax(X @ W, dim=1)[7] - 1.0 / k).abs().max()) < 1e-15
    zero = torch.zeros((), dtype=torch.float64)
    up = (F * torch.where(keep[:, None], gF, zero)).sum()
    if gt is not None:
        up = up + (T * torch.where(keep[:, None], gt, zero)).sum()
    a_X, a_W = torch.autograd.grad(up, (x, w))
    dirty = lambda t: None if t is None else torch.where(keep[:, None], t, nan)  # noqa: E731
    gX, gW = ref.intent_grads64(dirty(X), W, dirty(Z), dirty(gF), dirty(gt), rows=rows)
    assert torch.isfinite(gX).all() and torch.isfinite(gW).all() and gW.shape == (d, k)
    assert (gX[~keep] == 0).all()
    for name, got, want in (("gX", gX[keep], a_X[keep]), ("gW", gW, a_W)):
        err = float((got - want).abs().max() / want.abs().max())
        print("%s %s: closed form vs autograd %.3g of the largest entry" % (case, name, err))
        assert err <= 1e-12


def test_self_contrast_is_the_sum_of_both_arguments_gradients():
    """get_InfoNCE_loss(a, a, t): d / d a is the sum of the gradients of both arguments — what one panel as g1 and g2 of
    idg_infonce_pair_f32 receives."""
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(20, 64, dtype=torch.float64, generator=gen)
    x = a.clone().requires_grad_(True)
    (g_self,) = torch.autograd.grad(ref.infonce64(x, x, 0.2), x)
    u, v = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    g1, g2 = torch.autograd.grad(ref.infonce64(u, v, 0.2), (u, v))
    assert float((g_self - (g1 + g2)).abs().max()) <= 1e-15 and float(g_self.abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_has_every_key_the_plugin_reads():
    cfg = _cfg()
    assert dict(cfg) == KEYS and list(dict(cfg)) == list(KEYS)
    src = open(os.path.join(ROOT, "models", "BIGCF.py")).read() + open(os.path.join(ROOT, "id-grec_amd", "modeling.py")).read()
    read = set(re.findall(r"config\[['\"](\w+)['\"]\]", src))
    assert {"embedding_size", "intent_size", "GCN_layer", "reg_lambda", "ssl_lambda", "ssl_temperature", "int_temperature"} <= read
    assert read <= set(KEYS), read - set(KEYS)
    import utility.utility_function.tools as tools

    common = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    assert set(common) <= set(KEYS)  # the common keys of configure/LightGCN.txt are all there
    if os.path.isdir(os.path.join(REF, "configure")):
        assert not os.path.exists(os.path.join(REF, "configure", "BIGCF.txt"))  # the values are this project's choice


def test_plugin_resolves_and_refuses_what_it_cannot_run(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    mod = importlib.import_module("models.BIGCF")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.BIGCF
    assert cls.supports_fused_step and cls.n_fused_losses == 3 and cls.include_layer0 is False
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels"):
        assert callable(getattr(cls, name)), name
    from idgrec_amd.modeling import PackedRecommender

    assert issubclass(cls, PackedRecommender) and cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="BIGCF needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))


def test_constructor_draws_in_the_references_order():
    """The reference constructs its four nn.Embedding and initialises them afterwards; the plugin's base class initialises
    the two tables at once.  The constructor replays the reference's order of draws: stated here on plain torch."""
    from torch import nn

    U, I, d, k = 30, 25, 64, 128
    torch.manual_seed(2024)
    embs = [nn.Embedding(r, c) for r, c in ((U, d), (I, d), (d, k), (d, k))]
    want = [nn.init.xavier_uniform_(e.weight, gain=1.).detach().clone() for e in embs]
    torch.manual_seed(2024)
    rng = torch.get_rng_state()
    ue, ie = nn.Embedding(U, d), nn.Embedding(I, d)
    nn.init.xavier_uniform_(ue.weight, gain=1)
    nn.init.xavier_uniform_(ie.weight, gain=1)
    torch.set_rng_state(rng)
    for w in (ue.weight, ie.weight):
        torch.empty(w.shape).normal_()
    ui, ii = nn.Embedding(d, k), nn.Embedding(d, k)
    got = [nn.init.xavier_uniform_(e.weight, gain=1.).detach() for e in (ue, ie, ui, ii)]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    src = open(os.path.join(ROOT, "models", "BIGCF.py")).read()
    assert "torch.set_rng_state(rng)" in src and "torch.empty(w.shape).normal_()" in src


def test_main_names_bigcf_as_implemented():
    assert "BIGCF" in re.split(r"[,.\s]+", open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0])


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_intent_noise_f32", 7), ("idg_intent_fwd_f32", 17), ("idg_intent_bwd_workspace_bytes", 2),
                ("idg_intent_bwd_f32", 21))


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1)) == 142
    for name, n_args in ENTRY_POINTS:
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(native.PROTOTYPES[name][1]), name
        assert hasattr(native.lib, name)
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_intent.hip"' in build.split("SOURCES")[1].split("]")[0]
    assert native.lib.idg_intent_bwd_workspace_bytes(64, 128) == 256 * 64 * 128 * 4
    for d, k in ((0, 128), (32, 128), (64, 64), (64, 16), (128, 128), (-64, 128), (128, 64)):
        assert native.lib.idg_intent_bwd_workspace_bytes(d, k) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    # 10 x 64 floats = 2560 bytes per panel; with ld = 256: (9 * 256 + 64) * 4 = 9472 bytes; W 32768 bytes; the workspace
    # 8,388,608 bytes; the bitmap words of rows 0 .. 9: 4 bytes
    X0, W0, R0, Z0, T0, F0, N0, G0, H0, Q0, R1, WS0 = tuple(0x10000 * i for i in range(1, 12)) + (0x1000000,)

    def fwd(X=X0, ldx=64, row0=0, nrows=10, W=W0, d=64, k=128, rows=R0, noise=Z0, T=T0, ldt=64, F=F0, ldf=64, noise_out=N0):
        return L.idg_intent_fwd_f32(X, ldx, row0, nrows, W, d, k, rows, noise, 1234, 7, T, ldt, F, ldf, noise_out, None)

    def bwd(gF=G0, ldgf=64, gT=H0, ldgt=64, gt_rows=R1, rows=R0, X=X0, ldx=64, row0=0, nrows=10, W=W0, d=64, k=128, noise=Z0, gX=T0,
            ldgx=64, gW=Q0, ws=WS0):
        return L.idg_intent_bwd_f32(gF, ldgf, gT, ldgt, gt_rows, rows, X, ldx, row0, nrows, W, d, k, noise, 1234, 7, gX, ldgx, gW, ws, None)

    sizes = ((dict(nrows=0), "bad sizes"), (dict(nrows=-4), "bad sizes"), (dict(nrows=1 << 31), "bad sizes"), (dict(row0=-1), "bad sizes"),
             (dict(row0=(1 << 31) - 5), "bad sizes"), (dict(d=0), "(64, 128) only (got (0, 128))"), (dict(d=32), "(64, 128) only"),
             (dict(d=128), "(64, 128) only"), (dict(k=64), "(64, 128) only (got (64, 64))"), (dict(k=0), "(64, 128) only"),
             (dict(k=256), "(64, 128) only"), (dict(d=128, k=64), "(64, 128) only"))
    cases = {
        fwd: ((dict(X=None), "NULL"), (dict(W=None), "NULL"), (dict(T=None), "NULL"), (dict(F=None), "NULL"),
              (dict(X=X0 + 4), "misaligned"), (dict(W=W0 + 8), "misaligned"), (dict(T=T0 + 4), "misaligned"), (dict(F=F0 + 8), "misaligned"),
              (dict(noise=Z0 + 4), "misaligned"), (dict(noise_out=N0 + 12), "misaligned"), (dict(rows=R0 + 2), "misaligned"),
              (dict(ldx=60), "leading dimension"), (dict(ldt=66), "leading dimension"), (dict(ldf=0), "leading dimension"),
              (dict(ldx=1 << 20), "leading dimension"), (dict(ldf=-64), "leading dimension"),
              (dict(T=X0), "overlaps an input"), (dict(T=X0 + 2544), "overlaps an input"), (dict(F=X0 - 2544), "overlaps an input"),
              (dict(F=X0 - 9472 + 16, ldf=256), "overlaps an input"), (dict(T=W0 + 32752), "overlaps an input"), (dict(F=W0 - 16), "overlaps an input"),
              (dict(noise_out=Z0), "overlaps an input"), (dict(noise_out=X0 + 16), "overlaps an input"), (dict(T=R0), "overlaps an input"),
              (dict(T=Z0 + 16), "overlaps an input"), (dict(T=F0), "two outputs overlap"), (dict(F=T0 + 2544), "two outputs overlap"),
              (dict(noise_out=F0 + 16), "two outputs overlap"),
              # the spans start at row0: rows 5 .. 14 of T meet rows 0 .. 9 of a panel 1280 bytes further on
              (dict(T=X0 - 1280, row0=5, X=X0 - 5 * 256), "overlaps an input")),
        bwd: ((dict(gF=None), "NULL"), (dict(X=None), "NULL"), (dict(W=None), "NULL"), (dict(gX=None), "NULL"), (dict(gW=None), "NULL"),
              (dict(ws=None), "NULL"),
              (dict(gF=G0 + 4), "misaligned"), (dict(gT=H0 + 8), "misaligned"), (dict(X=X0 + 4), "misaligned"), (dict(W=W0 + 8), "misaligned"),
              (dict(noise=Z0 + 4), "misaligned"), (dict(gX=T0 + 4), "misaligned"), (dict(gW=Q0 + 2), "misaligned"), (dict(rows=R0 + 1), "misaligned"),
              (dict(gt_rows=R1 + 2), "misaligned"), (dict(ws=WS0 + 2), "misaligned"),
              (dict(ldgf=60), "leading dimension"), (dict(ldgt=66), "leading dimension"), (dict(ldx=0), "leading dimension"),
              (dict(ldgx=1 << 20), "leading dimension"),
              (dict(gX=G0), "overlaps an input"), (dict(gX=H0 + 16), "overlaps an input"), (dict(gX=X0 + 2544), "overlaps an input"),
              (dict(gX=W0), "overlaps an input"), (dict(gX=Z0), "overlaps an input"), (dict(gW=W0 + 32764), "overlaps an input"),
              (dict(gW=R0), "overlaps an input"), (dict(gW=R1 - 32764), "overlaps an input"), (dict(ws=X0 - 4096), "overlap"),
              (dict(ws=G0), "overlap"), (dict(gX=Q0 + 16), "two outputs overlap"), (dict(gW=WS0 + 4096), "two outputs overlap"),
              (dict(gX=WS0 + 8388608 - 16), "two outputs overlap")),
    }
    for fn, who in ((fwd, "idg_intent_fwd_f32"), (bwd, "idg_intent_bwd_f32")):
        for kw, word in cases[fn] + sizes:
            assert fn(**kw) == -1, (who, kw)
            msg = L.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)
    # gT_in absent: its leading dimension is not judged (the call is refused further on, for an output on top of W)
    assert bwd(gT=None, ldgt=0, gW=W0) == -1 and "overlaps an input" in L.idg_last_error().decode()
    for kw, word in ((dict(out=None), "NULL"), (dict(nrows=0), "bad sizes"), (dict(row0=-1), "bad sizes"), (dict(d=0), "bad sizes"),
                     (dict(d=1 << 20), "bad sizes")):
        a = dict(row0=0, nrows=10, d=64, out=N0)
        a.update(kw)
        assert L.idg_intent_noise_f32(a["row0"], a["nrows"], a["d"], 1234, 7, a["out"], None) == -1
        msg = L.idg_last_error().decode()
        assert "idg_intent_noise_f32" in msg and word in msg


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    X, W = torch.zeros(10, 64), torch.zeros(64, 128)
    for call in (lambda: ops.intent_mix(X, W), lambda: ops.intent_mix(torch.zeros(10, 32), torch.zeros(32, 16), stream=(1, 2)),
                 lambda: ops.intent_mix(X, W, noise=torch.zeros(10, 64))):
        with pytest.raises(RuntimeError, match="intent_mix: runs on MI355X only"):
            call()
    for call in (lambda: ops.intent_fwd_raw(X, W, torch.zeros(10, 64), torch.zeros(10, 64)),
                 lambda: ops.intent_bwd_raw(X, None, None, X, W, torch.zeros(10, 64), torch.zeros(64, 128)),
                 lambda: ops.intent_noise_raw(torch.zeros(10, 64), 1, 2)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    for bad in ((X.double(), W, None), (X, W.half(), None), (X, W, X.double())):
        with pytest.raises(TypeError, match="intent_mix: .* must be float32"):
            ops.intent_mix(bad[0], bad[1], noise=bad[2])
    with pytest.raises(ValueError, match=r"intent_mix: X must be \[n, d\]"):
        ops.intent_mix(torch.zeros(64), W)
    with pytest.raises(ValueError, match=r"intent_mix: X must be \[n, d\]"):
        ops.intent_mix(X, torch.zeros(64))
    with pytest.raises(ValueError, match="intent_mix: .* do not fit"):
        ops.intent_mix(torch.zeros(10, 32), W)
    with pytest.raises(ValueError, match="intent_mix: X has 0 rows"):
        ops.intent_mix(torch.zeros(0, 64), W)
    with pytest.raises(ValueError, match="intent_mix: noise .* must have X's shape"):
        ops.intent_mix(X, W, noise=torch.zeros(9, 64))
    with pytest.raises(ValueError, match="intent_mix: row0 = -1 is negative"):
        ops.intent_mix(X, W, row0=-1)
