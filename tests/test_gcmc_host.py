"""GCMC, host side: the fixture regenerates from the reference and holds both settings; tests/gcmc_ref64.py — the float64
statement tests/test_gpu_gcmc.py holds the kernels against — reproduces the reference's losses, gradients and three-step Adam
trajectory; the settings file carries the reference's keys; the plugin resolves through main.py's import path and does not
offer its fused step off the device or for a 128-wide layer; header / binding / library agree on the three entry points of
csrc/idg_gcmc.hip; every argument check of theirs comes before any device work; the wrapper's errors."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gcmc_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gcmc_small.npz")
# where the reference tree lives is stated once, by the golden generators (oracle/gen_golden.py)
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
REF_KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="1000", early_stopping="10",
                interval="10", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.0001",
                reg_lambda="0.0001", mess_dropout="True", mess_drop_prob="[0.1, 0.1, 0.1]", GCN_layer="1",
                layer_size="[64, 64, 64]", sparsity_test="0")
LAYERS = {"def": 1, "two": 2}
NAMES = ("W_gcn_%d", "b_gcn_%d", "W_mlp_%d", "b_mlp_%d")
RTOL = 1e-4  # tests/test_gccf_host.py
REG, LR = 1e-4, 1e-4  # configure/GCMC.txt, what the goldens were taken with


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "GCMC.txt"), "GCMC")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_gcmc.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    a, b = np.load(FIXTURE, allow_pickle=False), np.load(str(tmp_path / "gcmc_small.npz"), allow_pickle=False)
    assert sorted(a.keys()) == sorted(b.keys())
    for k in a.keys():  # every array byte for byte (the container's compressed stream is not compared)
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_fixture_holds_both_settings(golden_small):
    g = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert g["init_user"].shape == (300, 64) and g["init_item"].shape == (250, 64)
    for tag, K in LAYERS.items():
        n_small = 0
        for pre in ("", "grad_", "traj_"):
            for l in range(K):
                for nm in NAMES:
                    t = g["%s_%s%s" % (tag, pre, nm % l)]
                    assert t.shape == ((64, 64) if nm[0] == "W" else (1, 64)) and t.dtype == np.float32
                    assert np.isfinite(t).all() and np.abs(t).max() > 0
                    n_small += 1
            assert "%s_%sW_gcn_%d" % (tag, pre, K) not in g
        assert 2 + n_small // 3 == 2 + 4 * K  # two tables and K x (W_gcn, b_gcn, W_mlp, b_mlp)
        assert g[tag + "_loss"].shape == (2,) and g[tag + "_traj_loss"].shape == (3, 2)
        assert g[tag + "_grad_user"].shape == g[tag + "_traj_user"].shape == (300, 64)
        assert g[tag + "_grad_item"].shape == g[tag + "_traj_item"].shape == (250, 64)
        assert g[tag + "_rating"].shape == (32, 250)
        assert np.isfinite(g[tag + "_loss"]).all() and np.isfinite(g[tag + "_traj_user"]).all()
        # the rows that receive gradient are the batch's rows and what K products on the graph WITHOUT self loops reach
        gs = golden_small
        A = ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (550, 550)) != 0
        reach = torch.zeros(550, dtype=torch.bool)
        reach[torch.from_numpy(np.concatenate([g["batch"][:, 0], 300 + g["batch"][:, 1], 300 + g["batch"][:, 2]]))] = True
        for _ in range(K):
            reach = reach | ((A.double() @ reach.double()) > 0)
        got = np.concatenate([np.abs(g[tag + "_grad_user"]).sum(axis=1) > 0, np.abs(g[tag + "_grad_item"]).sum(axis=1) > 0])
        assert np.array_equal(got, reach.numpy())
    for nm in NAMES:
        assert np.array_equal(g["def_" + nm % 0], g["two_" + nm % 0])  # one seed, one creation order
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert g["traj_batches"].shape == (768, 3) and g["rating_users"].shape == (32,)


# ------------------------------------------------------------------------------- the float64 statement is the reference's
def _setting(golden_small, tag):
    g, gs = np.load(FIXTURE), golden_small
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (n, n))
    E0 = torch.from_numpy(np.concatenate([g["init_user"], g["init_item"]]))
    small = [tuple(torch.from_numpy(g["%s_%s" % (tag, nm % l)]) for nm in NAMES) for l in range(LAYERS[tag])]
    return g, U, A, E0, small


@pytest.mark.parametrize("tag", sorted(LAYERS))
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, U, A, E0, small = _setting(golden_small, tag)
    b = torch.from_numpy(g["batch"])
    losses, gE0, gsmall, final = ref.step64(A, E0, small, b[:, 0], b[:, 1], b[:, 2], None, REG, U)
    assert losses.dtype == gE0.dtype == final.dtype == torch.float64 and final.shape == (550, 64 * (LAYERS[tag] + 1))
    np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=RTOL)
    np.testing.assert_allclose(gE0[:U].numpy(), g[tag + "_grad_user"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(gE0[U:].numpy(), g[tag + "_grad_item"], rtol=1e-3, atol=1e-8)
    for l, layer in enumerate(gsmall):
        for nm, got in zip(NAMES, layer):
            np.testing.assert_allclose(got.numpy(), g["%s_grad_%s" % (tag, nm % l)], rtol=1e-3, atol=1e-7)
    # every normalised slot has unit rows; the reference's rating: sigmoid of the final rows' products
    for l in range(1, LAYERS[tag] + 1):
        assert torch.allclose(final[:, 64 * l:64 * (l + 1)].norm(dim=1), torch.ones(550, dtype=torch.float64), atol=1e-12)
    users = torch.from_numpy(g["rating_users"])
    np.testing.assert_allclose(torch.sigmoid(final[users] @ final[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    # the same expressions in float32: the yardstick the GPU file measures the kernels with
    l32, g32, s32, f32 = ref.step64(A, E0, small, b[:, 0], b[:, 1], b[:, 2], None, REG, U, dtype=torch.float32)
    assert l32.dtype == g32.dtype == s32[0][1].dtype == f32.dtype == torch.float32
    for name, a, x, y in (("d E0", g[tag + "_grad_item"], gE0[U:], g32[U:]), ("d W_gcn_0", g[tag + "_grad_W_gcn_0"], gsmall[0][0], s32[0][0]),
                          ("d b_mlp_0", g[tag + "_grad_b_mlp_0"], gsmall[0][3], s32[0][3])):
        e_ref, e_f32 = ref.errors(a, x, y)
        print("%s %s: the reference %.2e, the float32 composition %.2e of max from float64" % (tag, name, e_ref, e_f32))
        assert e_f32 < 1e-5


@pytest.mark.parametrize("tag", sorted(LAYERS))
def test_float64_statement_reproduces_the_references_trajectory(tag, golden_small):
    """Three step64 + adam64 steps on the fixture's three 256-row batches.  Losses at RTOL.  Parameters: the trajectory
    criterion of tests/test_gccf_host.py — fewer than one element in a thousand outside rtol 1e-4 / atol 1e-6, none further
    than 1e-4 (a third of the total movement: three Adam steps move an element by at most 3 lr = 3e-4)."""
    g, U, A, E0, small = _setting(golden_small, tag)
    K = LAYERS[tag]
    tri = torch.from_numpy(g["traj_batches"])
    flat0 = [E0.double()] + [t.double() for layer in small for t in layer]
    cur, grads, losses = list(flat0), [[] for _ in flat0], []
    for i in range(3):
        b = tri[i * 256:(i + 1) * 256]
        layers = [tuple(cur[1 + 4 * l: 5 + 4 * l]) for l in range(K)]
        ll, gE0, gsmall, _ = ref.step64(A, cur[0], layers, b[:, 0], b[:, 1], b[:, 2], None, REG, U)
        losses.append(ll.numpy())
        for k, t in enumerate([gE0] + [t for layer in gsmall for t in layer]):
            grads[k].append(t)
        cur = [ref.adam64(w0, gl, lr=LR)[-1][0] for w0, gl in zip(flat0, grads)]
    np.testing.assert_allclose(np.array(losses), g[tag + "_traj_loss"], rtol=RTOL)
    want = [np.concatenate([g[tag + "_traj_user"], g[tag + "_traj_item"]])]
    want += [g["%s_traj_%s" % (tag, nm % l)] for l in range(K) for nm in NAMES]
    for k, (mine, w) in enumerate(zip(cur, want)):
        mine = mine.numpy()
        assert mine.shape == w.shape
        moved = np.abs(w - flat0[k].numpy()).max()
        off = ~np.isclose(mine, w, rtol=1e-4, atol=1e-6)
        print("%s tensor %d: moved %.3g, off %.3g, max %.3g" % (tag, k, moved, off.mean(), np.abs(mine - w).max()))
        assert 1e-4 < moved <= 3.01 * LR
        assert off.mean() < 1e-3 and np.abs(mine - w).max() < 1e-4


def test_layer_conventions_at_the_kink_and_below_the_clamp():
    """What the kernels are held to where torch's own backward is a convention: the slope at H = 0 exactly, and the
    Jacobian I / 1e-12 on a row below the normalisation clamp."""
    n, d = 6, 64
    gen = torch.Generator().manual_seed(5)
    side = torch.randn(n, d, dtype=torch.float64, generator=gen)
    bg = torch.randn(d, dtype=torch.float64, generator=gen)
    side[2] = -bg  # Wg = I: H[2] = 0 exactly
    eye, one = torch.eye(d, dtype=torch.float64), torch.ones((), dtype=torch.float64)
    Wm, bm = torch.randn(d, d, dtype=torch.float64, generator=gen), torch.zeros(d, dtype=torch.float64)
    assert (ref.hidden64(side, eye, bg)[2] == 0).all()
    gE = torch.randn(n, d, dtype=torch.float64, generator=gen)
    g_side, _ = ref.layer_grads64(side, eye, bg, Wm, bm, one, gE, None)
    assert torch.allclose(g_side[2], ref.SLOPE * (gE[2] @ Wm.t()), rtol=1e-12, atol=0)
    tiny = torch.full((d,), 1e-13, dtype=torch.float64)
    T, N = ref.layer64(side, eye, bg, torch.zeros(d, d, dtype=torch.float64), tiny, one)
    assert torch.equal(T, tiny.expand(n, d)) and torch.allclose(N, T / 1e-12, rtol=1e-12, atol=0)
    _, flat = ref.layer_grads64(side, eye, bg, torch.zeros(d, d, dtype=torch.float64), tiny, one, None, gE)
    assert torch.allclose(flat[-d:], gE.sum(0) / 1e-12, rtol=1e-12, atol=0)  # gbm = column sums of gN / eps


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_carries_the_reference_keys():
    import utility.utility_function.tools as tools

    cfg = _cfg()
    assert dict(cfg) == REF_KEYS and list(dict(cfg)) == list(REF_KEYS)
    assert "node_dropout" not in cfg and "node_drop_prob" not in cfg
    if os.path.isdir(os.path.join(REF, "configure")):
        assert dict(tools.read_configuration(os.path.join(REF, "configure", "GCMC.txt"), "GCMC")) == REF_KEYS


def test_plugin_resolves_and_does_not_fuse_off_the_device(tmp_path, monkeypatch):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    from idgrec_amd.modeling import EngineStep, PackedRecommender

    mod = importlib.import_module("models.GCMC")  # main.py: importlib.import_module('models.' + model_name).Trainer
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.GCMC
    assert cls.supports_fused_step and cls.n_fused_losses == 2
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels"):
        assert callable(getattr(cls, name)), name
    assert issubclass(cls, PackedRecommender) and issubclass(cls, EngineStep)
    assert cls._eval_panels is not PackedRecommender._eval_panels and not hasattr(cls, "node_dropout")
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="GCMC needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))
    with pytest.raises(ValueError, match="fewer than GCN_layer"):
        cls(dict(cfg, GCN_layer="4"), data, torch.device("cpu"))
    # off the device the graph cannot be attached; with that step left out the model stands, on the CPU, and must not offer
    # its fused step — neither in the default setting nor with a 128-wide layer
    monkeypatch.setattr(PackedRecommender, "attach_graph", lambda self, sp_mat: None)
    torch.manual_seed(0)
    m = cls(cfg, data, torch.device("cpu"))
    assert list(m.weight_dict.keys()) == [nm % 0 for nm in NAMES] and len(list(m.parameters())) == 6
    assert not m._storage.is_cuda and m.fused_step_available() is False
    wide = cls(dict(cfg, GCN_layer="2", layer_size="[128, 64]"), data, torch.device("cpu"))
    assert [tuple(p.shape) for p in wide.weight_dict.values()] == [(64, 128), (1, 128), (128, 128), (1, 128), (128, 64), (1, 64),
                                                                  (64, 64), (1, 64)]
    assert wide.fused_step_available() is False
    # the same judgement with the storage claimed to be on the device: the 128-wide layer alone rules the fused step out
    class OnDevice:
        is_cuda, shape = True, (m._storage.shape[0], 64)

    monkeypatch.setattr(m, "_storage", OnDevice)
    monkeypatch.setattr(wide, "_storage", OnDevice)
    assert m.fused_step_available() is True and wide.fused_step_available() is False
    del m.mess_dropout  # mess_dropout = False in the settings: no attribute, no fused step
    assert m.fused_step_available() is False


def test_main_names_gcmc_as_implemented():
    assert "GCMC" in re.split(r"[,.\s]+", open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0])


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_gcmc_layer_fwd_f32", 15), ("idg_gcmc_layer_bwd_workspace_bytes", 1), ("idg_gcmc_layer_bwd_f32", 19))


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
    assert '"idg_gcmc.hip"' in build.split("SOURCES")[1].split("]")[0]
    assert native.lib.idg_gcmc_layer_bwd_workspace_bytes(64) == 512 * 2 * (64 * 64 + 64) * 4
    for d in (0, 32, 128, -64):
        assert native.lib.idg_gcmc_layer_bwd_workspace_bytes(d) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    # 10 x 64 floats = 2560 bytes per panel; a slot of a [10, 256] panel spans (9 * 256 + 64) * 4 = 9472 bytes; a matrix
    # 16384 bytes, a bias 256; [gWg | gbg | gWm | gbm] 33280 bytes; the workspace 17,039,360 bytes
    S0, WG0, BG0, WM0, BM0 = 0x10000, 0x20000, 0x30000, 0x34000, 0x3C000
    T0, N0, E0, R0, G0, Q0, WS0 = 0x40000, 0x50000, 0x58000, 0x60000, 0x80000, 0x90000, 0x1000000
    WSB = 17039360
    nan = float("nan")

    def fwd(side=S0, Wg=WG0, bg=BG0, Wm=WM0, bm=BM0, n=10, d=64, p=0.1, T=T0, N=N0, ldn=64):
        return L.idg_gcmc_layer_fwd_f32(side, Wg, bg, Wm, bm, n, d, 0.2, p, 1234, 7, T, N, ldn, None)

    def bwd(T=T0, gE=E0, gN=N0, ldgn=256, rows=R0, side=S0, Wg=WG0, bg=BG0, Wm=WM0, n=10, d=64, p=0.1, g_side=G0, w_grads=Q0,
            ws=WS0):
        return L.idg_gcmc_layer_bwd_f32(T, gE, gN, ldgn, rows, side, Wg, bg, Wm, n, d, 0.2, p, 1234, 7, g_side, w_grads, ws, None)

    sizes = ((dict(n=0), "bad sizes"), (dict(n=-4), "bad sizes"), (dict(n=1 << 31), "bad sizes"), (dict(d=0), "d = 64 only (got 0)"),
             (dict(d=32), "d = 64 only (got 32)"), (dict(d=128), "d = 64 only (got 128)"), (dict(d=-64), "d = 64 only"),
             (dict(p=-0.1), "drop probability"), (dict(p=1.0), "drop probability"), (dict(p=1.5), "drop probability"),
             (dict(p=nan), "drop probability"))
    cases = {
        fwd: ((dict(side=None), "NULL"), (dict(Wg=None), "NULL"), (dict(bg=None), "NULL"), (dict(Wm=None), "NULL"),
              (dict(bm=None), "NULL"), (dict(T=None), "NULL"), (dict(N=None), "NULL"),
              (dict(side=S0 + 4), "misaligned"), (dict(T=T0 + 8), "misaligned"), (dict(N=N0 + 4), "misaligned"),
              (dict(Wg=WG0 + 2), "misaligned"), (dict(bg=BG0 + 1), "misaligned"), (dict(Wm=WM0 + 3), "misaligned"),
              (dict(bm=BM0 + 2), "misaligned"), (dict(ldn=60), "leading dimension"), (dict(ldn=0), "leading dimension"),
              (dict(ldn=66), "leading dimension"), (dict(ldn=-64), "leading dimension"),
              (dict(T=S0), "overlaps"), (dict(T=S0 + 16), "overlaps"), (dict(T=S0 + 2544), "overlaps"), (dict(T=S0 - 2544), "overlaps"),
              (dict(N=S0), "overlaps"), (dict(N=S0 - 9472 + 16, ldn=256), "overlaps"), (dict(N=WG0 + 256), "overlaps"),
              (dict(T=WG0 - 16), "overlaps"), (dict(N=BG0), "overlaps"), (dict(T=BG0 + 240), "overlaps"), (dict(T=WM0 + 16368), "overlaps"),
              (dict(N=WM0 - 2544), "overlaps"), (dict(T=BM0), "overlaps"), (dict(N=BM0 + 240), "overlaps"),
              (dict(N=T0), "overlap"), (dict(N=T0 + 2544), "overlap"), (dict(N=T0 - 9472 + 16, ldn=256), "overlap")),
        bwd: ((dict(gE=None, gN=None), "NULL"), (dict(T=None), "NULL"), (dict(side=None), "NULL"), (dict(Wg=None), "NULL"),
              (dict(bg=None), "NULL"), (dict(Wm=None), "NULL"), (dict(g_side=None), "NULL"), (dict(w_grads=None), "NULL"),
              (dict(ws=None), "NULL"),
              (dict(T=T0 + 4), "misaligned"), (dict(gE=E0 + 4), "misaligned"), (dict(gN=N0 + 8), "misaligned"),
              (dict(side=S0 + 4), "misaligned"), (dict(Wg=WG0 + 8), "misaligned"), (dict(Wm=WM0 + 4), "misaligned"),
              (dict(bg=BG0 + 2), "misaligned"), (dict(g_side=G0 + 4), "misaligned"), (dict(w_grads=Q0 + 2), "misaligned"),
              (dict(rows=R0 + 1), "misaligned"), (dict(ws=WS0 + 2), "misaligned"),
              (dict(ldgn=60), "leading dimension"), (dict(ldgn=66), "leading dimension"), (dict(ldgn=0), "leading dimension"),
              (dict(ldgn=1 << 20), "leading dimension"),
              (dict(g_side=T0), "overlaps"), (dict(g_side=E0), "overlaps"), (dict(g_side=S0 + 16), "overlaps"),
              (dict(g_side=N0 + 64), "overlaps"), (dict(g_side=N0 + 9472 - 16), "overlaps"), (dict(g_side=WG0), "overlaps"),
              (dict(g_side=WM0 + 16368), "overlaps"), (dict(g_side=BG0 + 240), "overlaps"), (dict(w_grads=WG0), "overlaps"),
              (dict(w_grads=R0), "overlaps"), (dict(w_grads=R0 - 33276), "overlaps"), (dict(w_grads=T0 - 33276), "overlaps"),
              (dict(ws=S0 - 4096), "overlap"), (dict(ws=E0, gE=None), "overlap"), (dict(T=WS0 + WSB - 16), "overlap"),
              (dict(g_side=Q0 + 16), "overlap"), (dict(w_grads=WS0 + 4096), "overlap"), (dict(g_side=WS0 + WSB - 16), "overlap")),
    }
    for fn, who in ((fwd, "idg_gcmc_layer_fwd_f32"), (bwd, "idg_gcmc_layer_bwd_f32")):
        for kw, word in cases[fn] + sizes:
            assert fn(**kw) == -1, (who, kw)
            msg = L.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    side, W, b = torch.zeros(10, 64), torch.zeros(64, 64), torch.zeros(1, 64)
    for call in (lambda: ops.gcmc_layer(side, W, b, W, b, 0.1),
                 lambda: ops.gcmc_layer(torch.zeros(10, 128), torch.zeros(128, 64), torch.zeros(64), W, b, 0.0, stream=(1, 2)),
                 lambda: ops.gcmc_layer_fwd_raw(side, W, b, W, b, 0.1, 1, 2, torch.zeros(10, 64), torch.zeros(10, 64)),
                 lambda: ops.gcmc_layer_bwd_raw(side, side, None, 64, None, side, W, b, W, 0.1, 1, 2, torch.zeros(10, 64),
                                                torch.zeros(8320))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    for bad in ((side.double(), W, b, W, b), (side, W.half(), b, W, b), (side, W, b.double(), W, b), (side, W, b, W.double(), b),
                (side, W, b, W, b.half())):
        with pytest.raises(TypeError, match="float32"):
            ops.gcmc_layer(*bad, 0.1)
    with pytest.raises(ValueError, match=r"side must be \[n, d\]"):
        ops.gcmc_layer(torch.zeros(64), W, b, W, b, 0.1)
    with pytest.raises(ValueError, match=r"side must be \[n, d\]"):
        ops.gcmc_layer(side, W, b, torch.zeros(64), b, 0.1)
    for bad in ((torch.zeros(10, 32), W, b, W, b), (side, W, torch.zeros(1, 32), W, b), (side, W, b, torch.zeros(128, 64), b),
                (side, W, b, W, torch.zeros(1, 32))):
        with pytest.raises(ValueError, match="do not fit"):
            ops.gcmc_layer(*bad, 0.1)
    with pytest.raises(ValueError, match="0 rows"):
        ops.gcmc_layer(torch.zeros(0, 64), W, b, W, b, 0.1)
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError, match="drop probability"):
            ops.gcmc_layer(side, W, b, W, b, p)
