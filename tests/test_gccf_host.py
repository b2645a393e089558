"""LR-GCCF, host side: the fixture regenerates from the reference and holds both settings; tests/gccf_ref64.py — the float64
statement tests/test_gpu_gccf.py holds the kernels against — reproduces the reference's losses, gradients and three-step Adam
trajectory, and its closed-form layer gradients equal float64 autograd; the settings file carries the reference's keys; the
plugin resolves and refuses what it cannot run; header / binding / library agree on the three entry points of
csrc/idg_gccf.hip; every argument check of theirs comes before any device work; the wrapper's errors."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gccf_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gccf_small.npz")
# where the reference tree lives is stated once, by the golden generators (oracle/gen_golden.py)
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
REF_KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[20, 40]", training_epochs="1000", early_stopping="10",
                interval="10", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.0001",
                reg_lambda="0.0001", mess_dropout="True", mess_drop_prob="[0.1, 0.1, 0.1]", node_dropout="False",
                node_drop_prob="0.1", GCN_layer="3", layer_size="[64, 64, 64]", sparsity_test="0")
LAYERS = {"def": 3, "one": 1}
RTOL = 1e-4  # tests/test_ngcf_ref.py
REG, LR = 1e-4, 1e-4  # configure/GCCF.txt, what the goldens were taken with


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "GCCF.txt"), "GCCF")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_gccf.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    a, b = np.load(FIXTURE, allow_pickle=False), np.load(str(tmp_path / "gccf_small.npz"), allow_pickle=False)
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
                W, b = g["%s_%sW_gcn_%d" % (tag, pre, l)], g["%s_%sb_gcn_%d" % (tag, pre, l)]
                assert W.shape == (64, 64) and b.shape == (1, 64) and W.dtype == b.dtype == np.float32
                assert np.isfinite(W).all() and np.isfinite(b).all() and np.abs(W).max() > 0 and np.abs(b).max() > 0
                n_small += 2
            assert "%s_%sW_gcn_%d" % (tag, pre, K) not in g
        assert 2 + n_small // 3 == 2 + 2 * K  # two tables and K x (W, b): 8 parameter tensors in the default setting
        assert g[tag + "_loss"].shape == (2,) and g[tag + "_traj_loss"].shape == (3, 2)
        assert g[tag + "_grad_user"].shape == g[tag + "_traj_user"].shape == (300, 64)
        assert g[tag + "_grad_item"].shape == g[tag + "_traj_item"].shape == (250, 64)
        assert g[tag + "_rating"].shape == (32, 250)
        assert np.isfinite(g[tag + "_loss"]).all() and np.isfinite(g[tag + "_traj_user"]).all()
        # the rows that receive gradient are the batch's rows and what K products reach from them: with K = 3 every user and
        # all items but the four without a training edge, with K = 1 the batch and its neighbours
        gs = golden_small
        A = ref.dense_operator(gs["adjself_indptr"], gs["adjself_indices"], gs["adjself_data"], (550, 550)) != 0
        reach = torch.zeros(550, dtype=torch.bool)
        reach[torch.from_numpy(np.concatenate([g["batch"][:, 0], 300 + g["batch"][:, 1], 300 + g["batch"][:, 2]]))] = True
        for _ in range(K):
            reach = reach | ((A.double() @ reach.double()) > 0)
        got = np.concatenate([np.abs(g[tag + "_grad_user"]).sum(axis=1) > 0, np.abs(g[tag + "_grad_item"]).sum(axis=1) > 0])
        assert np.array_equal(got, reach.numpy())
        assert (int(got[:300].sum()), int(got[300:].sum())) == {"def": (300, 246), "one": (274, 146)}[tag]
    assert np.array_equal(g["def_W_gcn_0"], g["one_W_gcn_0"])  # one seed, one creation order
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert g["traj_batches"].shape == (768, 3) and g["rating_users"].shape == (32,)


# ------------------------------------------------------------------------------- the float64 statement is the reference's
def _setting(golden_small, tag):
    g, gs = np.load(FIXTURE), golden_small
    U, n = int(gs["num_users"]), int(gs["num_users"]) + int(gs["num_items"])
    A = ref.dense_operator(gs["adjself_indptr"], gs["adjself_indices"], gs["adjself_data"], (n, n))
    E0 = torch.from_numpy(np.concatenate([g["init_user"], g["init_item"]]))
    small = [(torch.from_numpy(g["%s_W_gcn_%d" % (tag, l)]), torch.from_numpy(g["%s_b_gcn_%d" % (tag, l)]))
             for l in range(LAYERS[tag])]
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
    for l, (gW, gb) in enumerate(gsmall):
        np.testing.assert_allclose(gW.numpy(), g["%s_grad_W_gcn_%d" % (tag, l)], rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(gb.numpy(), g["%s_grad_b_gcn_%d" % (tag, l)], rtol=1e-3, atol=1e-7)
    # the reference's rating: sigmoid of the final rows' products
    users = torch.from_numpy(g["rating_users"])
    np.testing.assert_allclose(torch.sigmoid(final[users] @ final[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    # the same expressions in float32: the yardstick the GPU file measures the kernels with
    l32, g32, s32, f32 = ref.step64(A, E0, small, b[:, 0], b[:, 1], b[:, 2], None, REG, U, dtype=torch.float32)
    assert l32.dtype == g32.dtype == s32[0][1].dtype == f32.dtype == torch.float32
    for name, a, x, y in (("d E0", g[tag + "_grad_item"], gE0[U:], g32[U:]), ("d W_gcn_0", g[tag + "_grad_W_gcn_0"], gsmall[0][0], s32[0][0]),
                          ("d b_gcn_0", g[tag + "_grad_b_gcn_0"], gsmall[0][1], s32[0][1])):
        e_ref, e_f32 = ref.errors(a, x, y)
        print("%s %s: the reference %.2e, the float32 composition %.2e of max from float64" % (tag, name, e_ref, e_f32))
        assert e_f32 < 1e-5


@pytest.mark.parametrize("tag", sorted(LAYERS))
def test_float64_statement_reproduces_the_references_trajectory(tag, golden_small):
    """Three step64 + adam64 steps on the fixture's three 256-row batches.  Losses at test_ngcf_ref.py's RTOL.  Parameters:
    three Adam steps move an element by at most 3 lr = 3e-4, and Adam divides by sqrt(v), so where a gradient is of the
    order of its own float32 rounding error the reference's element moves visibly differently — the trajectory criterion of
    tests/test_gpu_cgcl.py / test_gpu_lgcnpp.py: fewer than one element in a thousand outside rtol 1e-4 / atol 1e-6, none
    further than 1e-4 (a third of the total movement)."""
    g, U, A, E0, small = _setting(golden_small, tag)
    tri = torch.from_numpy(g["traj_batches"])
    flat0 = [E0.double()] + [t.double() for layer in small for t in layer]
    cur, grads, losses = list(flat0), [[] for _ in flat0], []
    for i in range(3):
        b = tri[i * 256:(i + 1) * 256]
        layers = [(cur[1 + 2 * l], cur[2 + 2 * l]) for l in range(LAYERS[tag])]
        ll, gE0, gsmall, _ = ref.step64(A, cur[0], layers, b[:, 0], b[:, 1], b[:, 2], None, REG, U)
        losses.append(ll.numpy())
        for k, t in enumerate([gE0] + [t for layer in gsmall for t in layer]):
            grads[k].append(t)
        cur = [ref.adam64(w0, gl, lr=LR)[-1][0] for w0, gl in zip(flat0, grads)]
    np.testing.assert_allclose(np.array(losses), g[tag + "_traj_loss"], rtol=RTOL)
    want = [np.concatenate([g[tag + "_traj_user"], g[tag + "_traj_item"]])]
    want += [g["%s_traj_%s_gcn_%d" % (tag, nm, l)] for l in range(LAYERS[tag]) for nm in ("W", "b")]
    for k, (mine, w) in enumerate(zip(cur, want)):
        mine = mine.numpy()
        assert mine.shape == w.shape
        moved = np.abs(w - flat0[k].numpy()).max()
        off = ~np.isclose(mine, w, rtol=1e-4, atol=1e-6)
        print("%s tensor %d: moved %.3g, off %.3g, max %.3g" % (tag, k, moved, off.mean(), np.abs(mine - w).max()))
        assert 1e-4 < moved <= 3.01 * LR
        assert off.mean() < 1e-3 and np.abs(mine - w).max() < 1e-4


@pytest.mark.parametrize("case", ["p=0.1", "a fully dropped row", "gN at two rows", "gE alone"])
def test_closed_form_layer_gradients_equal_float64_autograd(case):
    gen = torch.Generator().manual_seed(11)
    n, d = 50, 64
    side, W, b = (torch.randn(s, dtype=torch.float64, generator=gen) * 0.3 for s in ((n, d), (d, d), (1, d)))
    gE, gN = torch.randn(n, d, dtype=torch.float64, generator=gen), torch.randn(n, d, dtype=torch.float64, generator=gen)
    mask = ref.keep_mask(0.1, 1234, 7, n, d)
    assert 0.05 < float((mask == 0).double().mean()) < 0.15
    rows = None
    if case == "a fully dropped row":
        mask[3] = 0
    elif case == "gN at two rows":
        rows = [0, n - 1]
        keep = torch.zeros(n, dtype=torch.bool)
        keep[rows] = True
        gN = torch.where(keep[:, None], gN, torch.full_like(gN, float("nan")))
    elif case == "gE alone":
        gN = None
    s, w, bb = (x.clone().requires_grad_(True) for x in (side, W, b))
    E = ref.layer64(s, w, bb, mask)
    up = (E * gE).sum()
    if gN is not None:
        up = up + (E * torch.where(ref._flags(rows, n, "cpu")[:, None], gN, torch.zeros((), dtype=torch.float64))).sum()
    a_side, a_W, a_b = torch.autograd.grad(up, (s, w, bb))
    gT, g_side, flat = ref.layer_grads64(side, W, mask, gE, gN, gn_rows=rows)
    assert torch.isfinite(gT).all() and flat.shape == (d * d + d,)
    if case == "a fully dropped row":
        assert (E[3] == 0).all() and (gT[3] == 0).all() and (g_side[3] == 0).all()
    for name, got, want in (("g_side", g_side, a_side), ("gW", flat[:d * d].view(d, d), a_W), ("gb", flat[d * d:].view(1, d), a_b)):
        err = float((got - want).abs().max() / want.abs().max())
        print("%s %s: closed form vs autograd %.3g of the largest entry" % (case, name, err))
        assert err <= 1e-12


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_carries_the_reference_keys():
    import utility.utility_function.tools as tools

    cfg = _cfg()
    assert dict(cfg) == REF_KEYS and list(dict(cfg)) == list(REF_KEYS)
    if os.path.isdir(os.path.join(REF, "configure")):
        assert dict(tools.read_configuration(os.path.join(REF, "configure", "GCCF.txt"), "GCCF")) == REF_KEYS


def test_plugin_resolves_and_refuses_what_it_cannot_run(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    mod = importlib.import_module("models.GCCF")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.GCCF
    assert cls.supports_fused_step and cls.n_fused_losses == 2
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels"):
        assert callable(getattr(cls, name)), name
    from idgrec_amd.modeling import PackedRecommender

    assert issubclass(cls, PackedRecommender) and cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="GCCF needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))
    assert "node_keep_prob" not in cfg
    with pytest.raises(ValueError, match="node_keep_prob"):
        cls(dict(cfg, node_dropout="True"), data, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="GCCF needs an MI355X"):  # with the key it gets as far as the device
        cls(dict(cfg, node_dropout="True", node_keep_prob="0.9"), data, torch.device("cpu"))


def test_main_names_gccf_as_implemented():
    assert "GCCF" in re.split(r"[,.\s]+", open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0])


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_gccf_layer_fwd_f32", 11), ("idg_gccf_layer_bwd_workspace_bytes", 1), ("idg_gccf_layer_bwd_f32", 15))


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
    assert '"idg_gccf.hip"' in build.split("SOURCES")[1].split("]")[0]
    assert native.lib.idg_gccf_layer_bwd_workspace_bytes(64) == 512 * (64 * 64 + 64) * 4
    for d in (0, 32, 128, -64):
        assert native.lib.idg_gccf_layer_bwd_workspace_bytes(d) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    # 10 x 64 floats = 2560 bytes per panel; a slot of a [10, 256] panel spans (9 * 256 + 64) * 4 = 9472 bytes; W 16384 bytes;
    # [gW | gb] 16640 bytes; the workspace 8,519,680 bytes
    S0, W0, B0, E0, N0, R0, G0, Q0, WS0 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x80000, 0x90000, 0x100000
    nan = float("nan")

    def fwd(side=S0, W=W0, b=B0, n=10, d=64, p=0.1, E=E0, lde=64):
        return L.idg_gccf_layer_fwd_f32(side, W, b, n, d, p, 1234, 7, E, lde, None)

    def bwd(gE=E0, gN=N0, ldgn=256, rows=R0, side=S0, W=W0, n=10, d=64, p=0.1, g_side=G0, w_grads=Q0, ws=WS0):
        return L.idg_gccf_layer_bwd_f32(gE, gN, ldgn, rows, side, W, n, d, p, 1234, 7, g_side, w_grads, ws, None)

    sizes = ((dict(n=0), "bad sizes"), (dict(n=-4), "bad sizes"), (dict(n=1 << 31), "bad sizes"), (dict(d=0), "d = 64 only (got 0)"),
             (dict(d=32), "d = 64 only (got 32)"), (dict(d=128), "d = 64 only (got 128)"), (dict(d=-64), "d = 64 only"),
             (dict(p=-0.1), "drop probability"), (dict(p=1.0), "drop probability"), (dict(p=1.5), "drop probability"),
             (dict(p=nan), "drop probability"))
    cases = {
        fwd: ((dict(side=None), "NULL"), (dict(W=None), "NULL"), (dict(b=None), "NULL"), (dict(E=None), "NULL"),
              (dict(side=S0 + 4), "misaligned"), (dict(E=E0 + 8), "misaligned"), (dict(W=W0 + 2), "misaligned"),
              (dict(b=B0 + 1), "misaligned"), (dict(lde=60), "leading dimension"), (dict(lde=0), "leading dimension"),
              (dict(lde=66), "leading dimension"), (dict(lde=-64), "leading dimension"),
              (dict(E=S0), "overlaps"), (dict(E=S0 + 16), "overlaps"), (dict(E=S0 + 2544), "overlaps"), (dict(E=S0 - 2544), "overlaps"),
              (dict(E=S0 - 9472 + 16, lde=256), "overlaps"), (dict(E=W0 + 256), "overlaps"), (dict(E=W0 - 16), "overlaps"),
              (dict(E=B0), "overlaps"), (dict(E=B0 + 240), "overlaps")),
        bwd: ((dict(gE=None, gN=None), "NULL"), (dict(side=None), "NULL"), (dict(W=None), "NULL"), (dict(g_side=None), "NULL"),
              (dict(w_grads=None), "NULL"), (dict(ws=None), "NULL"),
              (dict(gE=E0 + 4), "misaligned"), (dict(gN=N0 + 8), "misaligned"), (dict(side=S0 + 4), "misaligned"),
              (dict(W=W0 + 8), "misaligned"), (dict(g_side=G0 + 4), "misaligned"), (dict(w_grads=Q0 + 2), "misaligned"),
              (dict(rows=R0 + 1), "misaligned"), (dict(ws=WS0 + 2), "misaligned"),
              (dict(ldgn=60), "leading dimension"), (dict(ldgn=66), "leading dimension"), (dict(ldgn=0), "leading dimension"),
              (dict(ldgn=1 << 20), "leading dimension"),
              (dict(g_side=E0), "overlaps"), (dict(g_side=S0 + 16), "overlaps"), (dict(g_side=N0 + 64), "overlaps"),
              (dict(g_side=N0 + 9472 - 16), "overlaps"), (dict(g_side=W0), "overlaps"), (dict(w_grads=W0), "overlaps"),
              (dict(w_grads=R0), "overlaps"), (dict(w_grads=R0 - 16636), "overlaps"), (dict(ws=S0 - 4096), "overlap"),
              (dict(ws=E0, gE=None), "overlap"), (dict(g_side=Q0 + 16), "overlap"), (dict(w_grads=WS0 + 4096), "overlap"),
              (dict(g_side=WS0 + 8519680 - 16), "overlap")),
    }
    for fn, who in ((fwd, "idg_gccf_layer_fwd_f32"), (bwd, "idg_gccf_layer_bwd_f32")):
        for kw, word in cases[fn] + sizes:
            assert fn(**kw) == -1, (who, kw)
            msg = L.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    side, W, b = torch.zeros(10, 64), torch.zeros(64, 64), torch.zeros(1, 64)
    for call in (lambda: ops.gccf_layer(side, W, b, 0.1), lambda: ops.gccf_layer(torch.zeros(10, 128), torch.zeros(128, 128),
                                                                                torch.zeros(128), 0.0, stream=(1, 2)),
                 lambda: ops.gccf_layer_fwd_raw(side, W, b, 0.1, 1, 2, torch.zeros(10, 64)),
                 lambda: ops.gccf_layer_bwd_raw(side, None, 64, None, side, W, 0.1, 1, 2, torch.zeros(10, 64), torch.zeros(4160))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    for bad in ((side.double(), W, b), (side, W.half(), b), (side, W, b.double())):
        with pytest.raises(TypeError, match="float32"):
            ops.gccf_layer(*bad, 0.1)
    with pytest.raises(ValueError, match=r"side must be \[n, d\]"):
        ops.gccf_layer(torch.zeros(64), W, b, 0.1)
    with pytest.raises(ValueError, match=r"side must be \[n, d\]"):
        ops.gccf_layer(side, torch.zeros(64), b, 0.1)
    with pytest.raises(ValueError, match="do not fit"):
        ops.gccf_layer(torch.zeros(10, 32), W, b, 0.1)
    with pytest.raises(ValueError, match="do not fit"):
        ops.gccf_layer(side, W, torch.zeros(1, 32), 0.1)
    with pytest.raises(ValueError, match="0 rows"):
        ops.gccf_layer(torch.zeros(0, 64), W, b, 0.1)
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError, match="drop probability"):
            ops.gccf_layer(side, W, b, p)
