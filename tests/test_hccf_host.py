"""HCCF, host side: the fixtures regenerate from the reference and hold both settings; tests/hccf_ref64.py — the float64
statement tests/test_gpu_hccf.py holds the kernels against — fed the reference's RECORDED keep masks reproduces the
reference's losses, every gradient, the rating and the three-step Adam trajectory to the rounding of the stored float32
numbers; its closed-form backward (the order the fused chain runs) equals float64 autograd; the settings file parses to the
reference's values; header, binding and library agree on the entry points of csrc/idg_hyper.hip, and every argument check of
theirs comes before any device work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import hccf_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"def": os.path.join(ROOT, "tests", "golden", "hccf_small.npz"), "drop": os.path.join(ROOT, "tests", "golden", "hccf_small_drop.npz")}
# where the reference tree lives is stated once, by the golden generators (oracle/gen_golden.py)
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="50", interval="1", early_stopping="10",
            embedding_size="64", batch_size="2048", test_batch_size="200", learn_rate="0.001", reg_lambda="0.0001", GCN_layer="3",
            hyper_size="64", ssl_lambda="0.3", temperature="0.1", keeprate="1.0", sparsity_test="0")
SETTINGS = {"def": (1.0, 3), "drop": (0.5, 2)}  # keeprate, GCN_layer
PARAMS = ("user_embedding", "item_embedding", "user_hyper_emb", "item_hyper_emb")
REG, SSL, TEMP, LR = 1e-4, 0.3, 0.1, 1e-3  # configure/HCCF.txt, what the goldens were taken with
ROUND = 2.0 ** -23  # a stored float32 tensor: max |mine - golden| <= 2^-23 max |golden| (its rounding is half of that)
LOSS_RTOL = 1e-10   # far above float64 summation-order noise, far below float32


def _golden(tag):
    g = dict(np.load(FIXTURES["def"], allow_pickle=False))
    if tag != "def":
        g.update(np.load(FIXTURES[tag], allow_pickle=False))
    return g


def _masks(g, tag, name):
    key = "%s_masks_%s" % (tag, name)
    return ref.unpack_masks(g[key]) if key in g else None


def _close(name, mine, golden):
    golden = np.asarray(golden)
    err = float(np.abs(np.asarray(mine, dtype=np.float64) - golden.astype(np.float64)).max()) / float(np.abs(golden).max())
    print("%s: %.3g of the largest entry (allowed %.3g)" % (name, err, ROUND))
    assert err <= ROUND, name


# ------------------------------------------------------------------------------------------------------------ the fixtures
def test_fixtures_regenerate_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_hccf.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    for path in FIXTURES.values():
        a, b = np.load(path, allow_pickle=False), np.load(str(tmp_path / os.path.basename(path)), allow_pickle=False)
        assert sorted(a.keys()) == sorted(b.keys())
        for k in a.keys():  # every array byte for byte
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        assert open(path, "rb").read() == open(str(tmp_path / os.path.basename(path)), "rb").read()


def test_fixtures_hold_both_settings():
    for path in FIXTURES.values():
        assert os.path.getsize(path) <= (1 << 20)
    shared = np.load(FIXTURES["def"])
    assert shared["init_user_embedding"].shape == (300, 64) and shared["init_item_embedding"].shape == (250, 64)
    assert shared["init_user_hyper_emb"].shape == shared["init_item_hyper_emb"].shape == (64, 64)
    b = shared["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert shared["traj_batches"].shape == (768, 3) and shared["rating_users"].shape == (32,)
    for tag, (keep, K) in SETTINGS.items():
        g = _golden(tag)
        assert g[tag + "_loss"].shape == (3,) and g[tag + "_traj_loss"].shape == (3, 3) and g[tag + "_rating"].shape == (32, 250)
        assert g[tag + "_loss"].dtype == np.float64 and np.isfinite(g[tag + "_loss"]).all() and (g[tag + "_loss"] > 0).all()
        assert tuple(g[tag + "_hyper"]) == (keep, K, LR, REG, SSL, TEMP)
        for p in PARAMS:
            for pre in ("grad", "traj"):
                a = g["%s_%s_%s" % (tag, pre, p)]
                assert a.shape == g["init_" + p].shape and a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
            moved = np.abs(g["%s_traj_%s" % (tag, p)] - g["init_" + p]).max()
            assert 1e-4 < moved <= 3.01e-3  # three Adam steps at lr = 1e-3
    assert not any(k.startswith("def_masks") for k in shared.keys())  # keeprate = 1.0: every mask is all ones, none stored
    g = _golden("drop")
    for name, lead in (("fwd", (2,)), ("rating", (2,)), ("traj", (3, 2))):
        m = ref.unpack_masks(g["drop_masks_" + name])
        assert tuple(m.shape) == lead + (550, 64) and abs(float(m.float().mean()) - 0.5) < 0.02
    assert not torch.equal(_masks(g, "drop", "fwd")[0], _masks(g, "drop", "fwd")[1])


# ------------------------------------------------------------------------------- the float64 statement is the reference's
def _setting(golden_small, tag):
    g, gs = _golden(tag), golden_small
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (n, n))
    E0 = torch.from_numpy(np.concatenate([g["init_user_embedding"], g["init_item_embedding"]]))
    return g, U, A, E0, torch.from_numpy(g["init_user_hyper_emb"]), torch.from_numpy(g["init_item_hyper_emb"])


@pytest.mark.parametrize("tag", sorted(SETTINGS))
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, U, A, E0, Wu, Wi = _setting(golden_small, tag)
    keep, K = SETTINGS[tag]
    b = torch.from_numpy(g["batch"])
    args = (K, _masks(g, tag, "fwd"), keep, REG, SSL, TEMP, U)
    losses, (gE0, gWu, gWi), final, S, Y = ref.step64(A, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], *args)
    assert losses.dtype == gE0.dtype == final.dtype == torch.float64 and final.shape == (550, 64) and len(S) == len(Y) == K
    np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=LOSS_RTOL, atol=0)
    _close(tag + " d user_embedding", gE0[:U], g[tag + "_grad_user_embedding"])
    _close(tag + " d item_embedding", gE0[U:], g[tag + "_grad_item_embedding"])
    _close(tag + " d user_hyper_emb", gWu, g[tag + "_grad_user_hyper_emb"])
    _close(tag + " d item_hyper_emb", gWi, g[tag + "_grad_item_hyper_emb"])
    # the reference's rating drew masks of its own
    users = torch.from_numpy(g["rating_users"])
    fin = ref.aggregate64(A, E0, Wu, Wi, U, K, _masks(g, tag, "rating"), keep)[0]
    _close(tag + " rating", torch.sigmoid(fin[users] @ fin[U:].t()), g[tag + "_rating"])
    # the closed-form backward of the fused chain is the same gradient
    l2, grads2 = ref.step_closed64(A, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], *args)
    assert torch.equal(l2, losses)
    for name, got, want in zip(("d E0", "d W_u", "d W_i"), grads2, (gE0, gWu, gWi)):
        err = float((got - want).abs().max() / want.abs().max())
        print("%s %s: closed form vs autograd %.3g of the largest entry" % (tag, name, err))
        assert err <= 1e-12
    # the same expressions in float32: the yardstick the GPU file measures the kernels with
    l32, g32, f32_, _, _ = ref.step64(A, E0, Wu, Wi, b[:, 0], b[:, 1], b[:, 2], *args, dtype=torch.float32)
    assert l32.dtype == g32[0].dtype == f32_.dtype == torch.float32
    for name, x, y in (("d E0", gE0, g32[0]), ("d W_u", gWu, g32[1]), ("d W_i", gWi, g32[2])):
        e_f32 = ref.errors(y, x, y)[1]
        print("%s %s: the float32 composition %.2e of max from float64" % (tag, name, e_f32))
        assert e_f32 < 1e-3


@pytest.mark.parametrize("tag", sorted(SETTINGS))
def test_float64_statement_reproduces_the_references_adam_trajectory(tag, golden_small):
    g, U, A, E0, Wu, Wi = _setting(golden_small, tag)
    keep, K = SETTINGS[tag]
    tri = torch.from_numpy(g["traj_batches"])
    tm = _masks(g, tag, "traj")
    init = (E0, Wu, Wi)
    cur, grads, traj = init, ([], [], []), []
    for i in range(3):
        b = tri[i * 256:(i + 1) * 256]
        losses, gs, _, _, _ = ref.step64(A, cur[0], cur[1], cur[2], b[:, 0], b[:, 1], b[:, 2], K, None if tm is None else tm[i], keep, REG, SSL,
                                         TEMP, U)
        traj.append(losses.numpy())
        for lst, x in zip(grads, gs):
            lst.append(x)
        cur = tuple(ref.adam64(w, lst, lr=LR)[-1][0] for w, lst in zip(init, grads))
    np.testing.assert_allclose(np.stack(traj), g[tag + "_traj_loss"], rtol=LOSS_RTOL, atol=0)
    _close(tag + " user_embedding after 3 steps", cur[0][:U], g[tag + "_traj_user_embedding"])
    _close(tag + " item_embedding after 3 steps", cur[0][U:], g[tag + "_traj_item_embedding"])
    _close(tag + " user_hyper_emb after 3 steps", cur[1], g[tag + "_traj_user_hyper_emb"])
    _close(tag + " item_hyper_emb after 3 steps", cur[2], g[tag + "_traj_item_hyper_emb"])


@pytest.mark.parametrize("case", ["no mask", "mask, keep 0.5", "mask, keep 1", "a zero row"])
def test_closed_form_layer_gradients_equal_float64_autograd(case):
    gen = torch.Generator().manual_seed(11)
    n, d, h = 50, 64, 64
    E0, W, X, gY = (torch.randn(s, dtype=torch.float64, generator=gen) * a for s, a in
                    (((n, d), 0.3), ((d, h), 0.4), ((n, d), 0.5), ((n, d), 1.0)))
    mask, keep = None, 1.0
    if case.startswith("mask"):
        mask = torch.rand((n, h), generator=gen) < 0.5
        keep = 0.5 if "0.5" in case else 1.0
    if case == "a zero row":
        E0[7] = 0
    e, w, x = (t.clone().requires_grad_(True) for t in (E0, W, X))
    Y, L, H = ref.layer64(e, w, x, mask, keep)
    assert Y.shape == (n, d) and L.shape == (h, d) and H.shape == (n, h)
    if mask is not None:
        assert (H[~mask] == 0).all() and torch.equal(H[mask], (E0 @ W)[mask] / keep)
    a_E, a_W, a_X = torch.autograd.grad((Y * gY).sum(), (e, w, x))
    gL, addX, gHb = ref.layer_grads64(E0, W, X, gY, mask, keep)
    addE, gW = ref.close64(E0, W, gHb)
    assert gL.shape == (h, d)
    for name, got, want in (("gX", addX, a_X), ("gE0", addE, a_E), ("gW", gW, a_W)):
        err = float((got - want).abs().max() / want.abs().max())
        print("%s %s: closed form vs autograd %.3g of the largest entry" % (case, name, err))
        assert err <= 1e-12
    if case == "a zero row":
        assert (Y[7] == 0).all() and (addX[7] == 0).all()


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_parses_to_the_references_values():
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "HCCF.txt"), "HCCF")
    assert dict(cfg) == KEYS and list(dict(cfg)) == list(KEYS)
    src = open(os.path.join(ROOT, "models", "HCCF.py")).read() + open(os.path.join(ROOT, "id-grec_amd", "modeling.py")).read()
    read = set(re.findall(r"config\[['\"](\w+)['\"]\]", src))
    assert {"embedding_size", "hyper_size", "GCN_layer", "reg_lambda", "ssl_lambda", "temperature", "keeprate"} <= read
    assert read <= set(KEYS), read - set(KEYS)
    if os.path.exists(os.path.join(REF, "configure", "HCCF.txt")):
        theirs = tools.read_configuration(os.path.join(REF, "configure", "HCCF.txt"), "HCCF")
        assert dict(theirs) == dict(cfg)


def test_plugin_resolves_and_refuses_what_it_cannot_run(tmp_path):
    import importlib

    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    mod = importlib.import_module("models.HCCF")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.HCCF
    assert cls.supports_fused_step and cls.n_fused_losses == 3 and cls.mask_source is None
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels"):
        assert callable(getattr(cls, name)), name
    from idgrec_amd.modeling import PackedRecommender

    assert issubclass(cls, PackedRecommender) and cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "HCCF.txt"), "HCCF")
    cfg.update(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="HCCF needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for bad in (dict(GCN_layer="0"), dict(keeprate="0"), dict(keeprate="1.5")):
        with pytest.raises(ValueError, match="HCCF needs"):
            cls(dict(cfg, **bad), data, torch.device("cpu"))


def test_constructor_draws_in_the_references_order():
    """The reference constructs its four nn.Embedding and initialises them afterwards; the plugin's base class initialises
    the two tables at once.  The constructor replays the reference's order of draws: stated here on plain torch."""
    from torch import nn

    U, I, d, h = 30, 25, 64, 64
    torch.manual_seed(2024)
    embs = [nn.Embedding(r, c) for r, c in ((U, d), (I, d), (d, h), (d, h))]
    want = [nn.init.xavier_uniform_(e.weight, gain=1.).detach().clone() for e in embs]
    torch.manual_seed(2024)
    rng = torch.get_rng_state()
    ue, ie = nn.Embedding(U, d), nn.Embedding(I, d)
    nn.init.xavier_uniform_(ue.weight, gain=1)
    nn.init.xavier_uniform_(ie.weight, gain=1)
    torch.set_rng_state(rng)
    for w in (ue.weight, ie.weight):
        torch.empty(w.shape).normal_()
    uh, ih = nn.Embedding(d, h), nn.Embedding(d, h)
    got = [nn.init.xavier_uniform_(e.weight, gain=1.).detach() for e in (ue, ie, uh, ih)]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    src = open(os.path.join(ROOT, "models", "HCCF.py")).read()
    assert "torch.set_rng_state(rng)" in src and "torch.empty(w.shape).normal_()" in src


def test_main_names_hccf_as_implemented():
    assert "HCCF" in re.split(r"[,.\s]+", open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0])


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_hyper_latent_workspace_bytes", 2), ("idg_hyper_latent_f32", 17), ("idg_hyper_expand_f32", 21),
                ("idg_hyper_bwd_f32", 23), ("idg_hyper_close_workspace_bytes", 2), ("idg_hyper_close_f32", 14))


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    for name, n_args in ENTRY_POINTS:
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(native.PROTOTYPES[name][1]), name
        assert hasattr(native.lib, name)
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_hyper.hip"' in build.split("SOURCES")[1].split("]")[0]
    for fn in (native.lib.idg_hyper_latent_workspace_bytes, native.lib.idg_hyper_close_workspace_bytes):
        assert fn(64, 64) == 512 * 64 * 64 * 4
        for d, h in ((0, 64), (32, 16), (64, 128), (128, 64), (64, 32), (-64, 64)):
            assert fn(d, h) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    lib = native.lib
    # 10 x 64 floats = 2560 bytes per panel, a [64, 64] matrix 16384 bytes, 10 x 64 mask bytes = 640, the workspace 8,388,608
    E, W, X, Lm, GL, Y, S, N, T, M, MO, GH = tuple(0x10000 * i for i in range(1, 13))
    WS = 0x1000000

    def latent(E0=E, lde=64, W=W, d=64, h=64, X=X, ldx=64, row0=0, nrows=10, keep=0.5, mask=M, L=Lm, mask_out=MO, ws=WS):
        return lib.idg_hyper_latent_f32(E0, lde, W, d, h, X, ldx, row0, nrows, keep, mask, 1234, 7, L, mask_out, ws, None)

    def expand(E0=E, lde=64, W=W, d=64, h=64, L=Lm, row0=0, nrows=10, keep=0.5, mask=M, Y=Y, ldy=64, side=S, lds=64, next=N, ldn=64,
               total=T, ldtot=64):
        return lib.idg_hyper_expand_f32(E0, lde, W, d, h, L, row0, nrows, keep, mask, 1234, 7, Y, ldy, side, lds, next, ldn, total, ldtot, None)

    def bwd(E0=E, lde=64, W=W, d=64, h=64, X=X, ldx=64, gY=Y, ldgy=64, L=Lm, gL=GL, row0=0, nrows=10, keep=0.5, mask=M, gX=N, ldgx=64,
            gHb=GH, ldgh=64, accumulate=0):
        return lib.idg_hyper_bwd_f32(E0, lde, W, d, h, X, ldx, gY, ldgy, L, gL, row0, nrows, keep, mask, 1234, 7, gX, ldgx, gHb, ldgh,
                                     accumulate, None)

    def close(E0=E, lde=64, W=W, d=64, h=64, gHb=GH, ldgh=64, row0=0, nrows=10, gE0=N, ldge=64, gW=GL, ws=WS):
        return lib.idg_hyper_close_f32(E0, lde, W, d, h, gHb, ldgh, row0, nrows, gE0, ldge, gW, ws, None)

    sizes = ((dict(nrows=0), "bad sizes"), (dict(nrows=-4), "bad sizes"), (dict(nrows=1 << 31), "bad sizes"), (dict(row0=-1), "bad sizes"),
             (dict(row0=(1 << 31) - 5), "bad sizes"), (dict(d=0), "(64, 64) only (got (0, 64))"), (dict(d=32), "(64, 64) only"),
             (dict(d=128), "(64, 64) only"), (dict(h=128), "(64, 64) only (got (64, 128))"), (dict(h=0), "(64, 64) only"),
             (dict(d=32, h=16), "(64, 64) only"))
    keeps = ((dict(keep=0.0), "not positive"), (dict(keep=-0.5), "not positive"), (dict(keep=float("nan")), "not positive"))
    cases = {
        latent: keeps + (
            (dict(E0=None), "NULL"), (dict(W=None), "NULL"), (dict(X=None), "NULL"), (dict(L=None), "NULL"), (dict(ws=None), "NULL"),
            (dict(E0=E + 4), "misaligned"), (dict(W=W + 8), "misaligned"), (dict(X=X + 4), "misaligned"), (dict(L=Lm + 8), "misaligned"),
            (dict(ws=WS + 4), "misaligned"), (dict(mask=M + 2), "misaligned"), (dict(mask_out=MO + 1), "misaligned"),
            (dict(lde=60), "leading dimension"), (dict(ldx=66), "leading dimension"), (dict(ldx=0), "leading dimension"),
            (dict(lde=1 << 20), "leading dimension"),
            (dict(L=E), "overlaps an input"), (dict(L=X + 2544), "overlaps an input"), (dict(L=W + 16368), "overlaps an input"),
            (dict(L=M - 16368), "overlaps an input"), (dict(mask_out=M + 636), "overlaps an input"), (dict(mask_out=X), "overlaps an input"),
            (dict(ws=E - 4096), "overlaps an input"), (dict(mask_out=Lm + 16), "two outputs overlap"), (dict(L=WS + 4096), "two outputs overlap"),
            # the spans start at row0: rows 5 .. 14 of the mask written meet rows 0 .. 9 of the one read 320 bytes further on
            (dict(mask_out=M - 320, row0=5, mask=M - 5 * 64, E0=E - 5 * 256, X=X - 5 * 256), "overlaps an input")),
        expand: keeps + (
            (dict(E0=None), "NULL"), (dict(W=None), "NULL"), (dict(L=None), "NULL"), (dict(Y=None), "NULL"),
            (dict(side=None), "come together"), (dict(next=None), "come together"),
            (dict(E0=E + 4), "misaligned"), (dict(L=Lm + 4), "misaligned"), (dict(Y=Y + 8), "misaligned"), (dict(side=S + 4), "misaligned"),
            (dict(next=N + 4), "misaligned"), (dict(total=T + 12), "misaligned"), (dict(mask=M + 1), "misaligned"),
            (dict(lde=60), "leading dimension"), (dict(ldy=66), "leading dimension"), (dict(lds=32), "leading dimension"),
            (dict(ldn=-64), "leading dimension"), (dict(ldtot=1 << 20), "leading dimension"),
            (dict(Y=E), "overlaps an input"), (dict(Y=Lm + 16368), "overlaps an input"), (dict(next=S), "overlaps an input"),
            (dict(total=S + 2544), "overlaps an input"), (dict(total=W), "overlaps an input"), (dict(Y=M), "overlaps an input"),
            (dict(next=Y), "two outputs overlap"), (dict(total=Y + 2544), "two outputs overlap"), (dict(total=N - 2544), "two outputs overlap")),
        bwd: keeps + (
            (dict(E0=None), "NULL"), (dict(W=None), "NULL"), (dict(X=None), "NULL"), (dict(gY=None), "NULL"), (dict(L=None), "NULL"),
            (dict(gL=None), "NULL"), (dict(gX=None), "NULL"), (dict(gHb=None), "NULL"),
            (dict(X=X + 4), "misaligned"), (dict(gY=Y + 8), "misaligned"), (dict(gL=GL + 4), "misaligned"), (dict(gX=N + 4), "misaligned"),
            (dict(gHb=GH + 8), "misaligned"), (dict(mask=M + 3), "misaligned"),
            (dict(ldx=60), "leading dimension"), (dict(ldgy=66), "leading dimension"), (dict(ldgx=0), "leading dimension"),
            (dict(ldgh=1 << 20), "leading dimension"), (dict(lde=62), "leading dimension"),
            (dict(gX=X), "overlaps an input"), (dict(gX=Y + 2544), "overlaps an input"), (dict(gHb=E), "overlaps an input"),
            (dict(gHb=GL - 2544), "overlaps an input"), (dict(gX=Lm), "overlaps an input"), (dict(gHb=M), "overlaps an input"),
            (dict(gHb=N), "two outputs overlap"), (dict(gX=GH + 2544), "two outputs overlap")),
        close: (
            (dict(E0=None), "NULL"), (dict(W=None), "NULL"), (dict(gHb=None), "NULL"), (dict(gE0=None), "NULL"), (dict(gW=None), "NULL"),
            (dict(ws=None), "NULL"),
            (dict(E0=E + 4), "misaligned"), (dict(gHb=GH + 4), "misaligned"), (dict(gE0=N + 8), "misaligned"), (dict(gW=GL + 4), "misaligned"),
            (dict(ws=WS + 8), "misaligned"),
            (dict(lde=60), "leading dimension"), (dict(ldgh=66), "leading dimension"), (dict(ldge=0), "leading dimension"),
            (dict(gE0=E), "overlaps an input"), (dict(gE0=GH + 2544), "overlaps an input"), (dict(gW=W + 16368), "overlaps an input"),
            (dict(ws=GH), "overlaps an input"), (dict(gW=N + 16), "two outputs overlap"), (dict(gW=WS + 8388608 - 16), "two outputs overlap")),
    }
    for fn, who in ((latent, "idg_hyper_latent_f32"), (expand, "idg_hyper_expand_f32"), (bwd, "idg_hyper_bwd_f32"),
                    (close, "idg_hyper_close_f32")):
        for kw, word in cases[fn] + sizes:
            assert fn(**kw) == -1, (who, kw)
            msg = lib.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)
    # side and next absent together: their leading dimensions are not judged (the call is refused further on)
    assert expand(side=None, next=None, lds=0, ldn=0, Y=E) == -1 and "overlaps an input" in lib.idg_last_error().decode()


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    E0, W, X = torch.zeros(10, 64), torch.zeros(64, 64), torch.zeros(10, 64)
    for call in (lambda: ops.hyper_mix(E0, W, X), lambda: ops.hyper_mix(torch.zeros(10, 32), torch.zeros(32, 16), torch.zeros(10, 32)),
                 lambda: ops.hyper_mix(E0, W, X, mask=torch.ones(10, 64, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="hyper_mix: runs on MI355X only"):
            call()
    for call in (lambda: ops.hyper_latent_raw(E0, W, X, torch.zeros(64, 64)), lambda: ops.hyper_expand_raw(E0, W, W, torch.zeros(10, 64)),
                 lambda: ops.hyper_bwd_raw(E0, W, X, X, W, W, torch.zeros(10, 64), torch.zeros(10, 64)),
                 lambda: ops.hyper_close_raw(E0, W, X, torch.zeros(10, 64), torch.zeros(64, 64))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    for bad in ((E0.double(), W, X), (E0, W.half(), X), (E0, W, X.double())):
        with pytest.raises(TypeError, match="hyper_mix: .* must be float32"):
            ops.hyper_mix(*bad)
    for bad in ((torch.zeros(64), W, X), (E0, W, torch.zeros(9, 64)), (torch.zeros(10, 32), W, X)):
        with pytest.raises(ValueError, match="hyper_mix: .* do not fit"):
            ops.hyper_mix(*bad)
    with pytest.raises(ValueError, match="hyper_mix: E0 has 0 rows"):
        ops.hyper_mix(torch.zeros(0, 64), W, torch.zeros(0, 64))
    with pytest.raises(ValueError, match=r"hyper_mix: mask .* must be \[n, h\]"):
        ops.hyper_mix(E0, W, X, mask=torch.ones(9, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="hyper_mix: row0 = -1"):
        ops.hyper_mix(E0, W, X, row0=-1)
    with pytest.raises(ValueError, match="keep = 0 must be positive"):
        ops.hyper_mix(E0, W, X, keep=0.0)
