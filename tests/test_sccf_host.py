"""SCCF, host side: the fixture regenerates from the reference and holds both settings; tests/sccf_ref64.py — the float64
statement tests/test_gpu_sccf.py holds the kernels against — reproduces the reference's loss pair, both gradients and the
rating in its literal (torch.unique) and its collapsed (B x B) form, and the two forms agree; the float32 yardstick of the
GPU tests is measured and printed; the reference's own float32 run meets the trajectory criterion; the settings file
carries every key the plugin reads; header / binding / library agree on the entry points of csrc/idg_sccf.hip, and their
argument checks come before any device work.

The fixture is the reference's own program run in float64 from its float32 initial tables (scripts/gen_golden_sccf.py), so
the statement is held to it at rtol 1e-6 (losses) and 1e-6 of the largest entry (gradients).  Measured here: losses equal to
1e-16, gradients 4.0e-8 (`mf`) and 5.0e-8 (`gcn`) of their largest entry — the float32 rounding of the stored arrays; the
two forms agree to 1.3e-16 (losses) and 3.4e-15 (gradients).
The float32 yardstick (the literal form in float32 against the float64 statement; losses relative, gradients as a share of
the largest entry): fixture `mf` 6.6e-8 / 1.42e-6, `gcn` 1.6e-8 / 1.09e-6; worst over grid (a) of tests/test_gpu_sccf.py:
losses 1.42e-7, gradients 8.5e-7 (T = 0.1) and 4.1e-7 (T = 1); the cases riding on a few of its sizes: all-distinct ids
2.4e-7, zero rows 3.7e-7, store / accumulate 3.4e-7, and one user repeated B times 9.6e-7 (B = 96), 8.5e-7 (B = 257) and 2.11e-6
(B = 129, d = 48, T = 1: there the two terms' shares of the one user row's gradient nearly cancel, and the rounding of Z and of
the row sums is amplified about tenfold).  The worst gradient figure is 2.11e-6: twice that, rounded up to two digits, is
tests/test_gpu_sccf.py's GRAD_TOL = 4.3e-6 (tighter than the siblings' 1e-5, which caps it).  The cases over every built
width (tests/widths.py: EVERY_NDT at B = 129 and 257, T = 0.1): losses 1.2e-7, gradients 2.5e-7 .. 7.7e-7 (B = 257, d = 32). The
reference's own float32 run on the fixture's three batches: `mf` no element outside rtol 1e-4 / atol 1e-6 (8.9e-8 off at
most), `gcn` 2.8e-5 of the elements outside, 1.2e-5 off at most."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import sccf_ref64 as ref  # noqa: E402
from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sccf_small.npz")
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="300", interval="1",
            early_stopping="20", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.001",
            reg_lambda="0.0001", GCN_layer="3", temperature="0.1", encoder="MF", sparsity_test="0")
TAGS = ("mf", "gcn")
PARAMS = ("user_embedding", "item_embedding")
WORST_YARDSTICK = 2.15e-6  # what tests/test_gpu_sccf.py's GRAD_TOL = 4.3e-6 was taken from: a larger measurement must show


def _setting(g, tag):
    t, layers, lr = g[tag + "_hyper"].tolist()
    return float(t), int(layers), float(lr)


def _operator(tag, gs):
    n = int(gs["num_users"]) + int(gs["num_items"])
    return None if tag == "mf" else ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (n, n))


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_sccf.py")], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    assert open(FIXTURE, "rb").read() == open(str(tmp_path / "sccf_small.npz"), "rb").read()


def test_fixture_holds_both_settings():
    assert os.path.getsize(FIXTURE) < (1 << 20)
    g = np.load(FIXTURE, allow_pickle=False)
    assert g["init_user_embedding"].shape == (300, 64) and g["init_item_embedding"].shape == (250, 64)
    b = g["batch"]
    nu, ni = g["batch_counts"].tolist()
    assert b.shape == (96, 3) and nu == len(set(b[:, 0].tolist())) < 96 and ni == len(set(b[:, 1].tolist())) < 96
    assert g["traj_batches"].shape == (768, 3) and g["rating_users"].shape == (32,)
    assert _setting(g, "mf") == (0.1, 3, 1e-3) and _setting(g, "gcn") == (0.2, 2, 1e-3)
    for tag in TAGS:
        assert g[tag + "_loss"].shape == (2,) and g[tag + "_traj_loss"].shape == (3, 2) and g[tag + "_rating"].shape == (32, 250)
        assert g[tag + "_loss"].dtype == np.float64 and np.isfinite(g[tag + "_loss"]).all() and np.isfinite(g[tag + "_traj_loss"]).all()
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
    U = int(gs["num_users"])
    t, layers, _ = _setting(g, tag)
    A = _operator(tag, gs)
    E0 = torch.from_numpy(np.concatenate([g["init_user_embedding"], g["init_item_embedding"]]))
    b = torch.from_numpy(g["batch"])
    want = np.concatenate([g[tag + "_grad_user_embedding"], g[tag + "_grad_item_embedding"]])
    res = {}
    for collapsed in (False, True):
        losses, gE0, X = ref.step64(A, E0, b[:, 0], b[:, 1], layers, t, U, collapsed=collapsed)
        assert losses.dtype == gE0.dtype == X.dtype == torch.float64 and losses.shape == (2,) and gE0.shape == E0.shape
        e_loss = float(np.abs(losses.numpy() / g[tag + "_loss"] - 1).max())
        e_grad = float(np.abs(gE0.numpy() - want).max() / np.abs(want).max())
        print("%s (%s): losses %.2e (relative), gradients %.2e of the largest entry from the fixture"
              % (tag, "collapsed" if collapsed else "literal", e_loss, e_grad))
        np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=1e-6)
        assert e_grad <= 1e-6
        users = torch.from_numpy(g["rating_users"])
        np.testing.assert_allclose(torch.sigmoid(X[users] @ X[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-6, atol=1e-7)
        res[collapsed] = (losses, gE0)
    (l_l, g_l), (l_c, g_c) = res[False], res[True]
    e_l, e_g = float(((l_c - l_l) / l_l).abs().max()), float((g_c - g_l).abs().max() / g_l.abs().max())
    print("%s: collapsed against literal: losses %.2e, gradients %.2e" % (tag, e_l, e_g))
    assert e_l <= 1e-12 and e_g <= 1e-12


@pytest.mark.parametrize("form", ["distinct", "one_user"])
def test_the_two_forms_agree_on_edge_batches(form):
    """All ids distinct (Nu = Ni = B: the counts are all one) and one user repeated B times (Nu = 1)."""
    for B, d, t in ((37, 24, 0.1), (96, 64, 1.0)):
        panel, users, pos, U = ref.case_inputs(B, d, 11 + B, form=form)
        assert int(torch.unique(users).numel()) == (B if form == "distinct" else 1)
        l_l, g_l = ref.panel_terms(panel, U, users, pos, t)
        l_c, g_c = ref.panel_terms(panel, U, users, pos, t, collapsed=True)
        assert float(((l_c - l_l) / l_l).abs().max()) <= 1e-12
        assert float((g_c - g_l).abs().max()) <= 1e-12 * float(g_l.abs().max())


# ------------------------------------------------------------------------------------------------- the float32 yardstick
def _yardstick(panel, U, users, pos, t, A=None, layers=0, upstream=None):
    if A is None and layers == 0:
        l64, g64 = ref.panel_terms(panel, U, users, pos, t, upstream=upstream)
        l32, g32 = ref.panel_terms(panel, U, users, pos, t, dtype=torch.float32, upstream=upstream)
    else:
        l64, g64, _ = ref.step64(A, panel, users, pos, layers, t, U)
        l32, g32, _ = ref.step64(A, panel, users, pos, layers, t, U, dtype=torch.float32)
    return float(((l32.double() - l64) / l64).abs().max()), float((g32.double() - g64).abs().max() / g64.abs().max())


def test_float32_yardstick_is_measured(golden_small):
    """The largest distance of the float32 literal form from the float64 statement, over the fixture's inputs and every case
    of grid (a) of tests/test_gpu_sccf.py (the same seeds, on the CPU).  Printed; the docstring records the values."""
    g, gs = np.load(FIXTURE, allow_pickle=False), golden_small
    U = int(gs["num_users"])
    E0 = torch.from_numpy(np.concatenate([g["init_user_embedding"], g["init_item_embedding"]]))
    b = torch.from_numpy(g["batch"])
    worst_l, worst_g = 0.0, {0.1: 0.0, 1.0: 0.0}
    for tag in TAGS:
        t, layers, _ = _setting(g, tag)
        A = _operator(tag, gs)
        e_l, e_g = _yardstick(E0, U, b[:, 0], b[:, 1], t, A, 0 if A is None else layers)
        print("fixture %s: float32 literal form: losses %.2e, gradients %.2e of the largest entry" % (tag, e_l, e_g))
        assert e_l < 1e-5 and e_g <= WORST_YARDSTICK
    for B in ref.GRID_B:
        for d in ref.GRID_D:
            for t in ref.GRID_T:
                panel, users, pos, Uc = ref.case_inputs(B, d, ref.grid_seed(B, d, t))
                e_l, e_g = _yardstick(panel, Uc, users, pos, t, upstream=ref.grid_upstream(B))
                worst_l, worst_g[t] = max(worst_l, e_l), max(worst_g[t], e_g)
    print("grid (a): float32 literal form: losses %.2e; gradients %.2e (T = 0.1), %.2e (T = 1) of the largest entry"
          % (worst_l, worst_g[0.1], worst_g[1.0]))
    # the cases riding on a few of its sizes: distinct ids, one repeated user, zero rows (the live rows), store / accumulate
    for form, B, d, t, seed in ref.RIDERS:
        panel, users, pos, Uc = ref.case_inputs(B, d, seed, form=form)
        l64, g64 = ref.panel_terms(panel, Uc, users, pos, t)
        l32, g32 = ref.panel_terms(panel, Uc, users, pos, t, dtype=torch.float32)
        keep = torch.ones(panel.shape[0], dtype=torch.bool)
        if form == "zero_rows":
            keep[list(ref.zero_rows_of(users, pos, Uc))] = False
        e_l = float(((l32.double() - l64) / l64).abs().max())
        e_g = float((g32.double() - g64)[keep].abs().max() / g64[keep].abs().max())
        print("rider %s B=%d d=%d T=%g: losses %.2e, gradients %.2e of the largest entry" % (form, B, d, t, e_l, e_g))
        worst_l, worst_g[t] = max(worst_l, e_l), max(worst_g[t], e_g)
    print("grid (a) with its riders: losses %.2e; gradients %.2e (T = 0.1), %.2e (T = 1)" % (worst_l, worst_g[0.1], worst_g[1.0]))
    assert worst_l < 1e-5 and max(worst_g.values()) <= WORST_YARDSTICK


def test_float32_yardstick_over_every_built_width():
    """The same measurement on the cases tests/test_gpu_sccf.py runs over tests/widths.py's EVERY_NDT (the same seeds, on the
    CPU): none above the figure GRAD_TOL was taken from, so those cases take GRAD_TOL unchanged."""
    worst_l, worst_g = (0.0, None), (0.0, None)
    for B in ref.WIDTH_B:
        for d in widths.EVERY_NDT:
            panel, users, pos, Uc = ref.case_inputs(B, d, ref.width_seed(B, d))
            e_l, e_g = _yardstick(panel, Uc, users, pos, ref.WIDTH_T, upstream=ref.grid_upstream(B))
            print("widths B=%d d=%d T=%g: float32 literal form: losses %.2e, gradients %.2e of the largest entry" % (B, d, ref.WIDTH_T, e_l, e_g))
            worst_l, worst_g = max(worst_l, (e_l, (B, d))), max(worst_g, (e_g, (B, d)))
    print("every built width: losses %.2e (B, d = %s); gradients %.2e (B, d = %s)" % (worst_l + worst_g))
    assert worst_l[0] < 1e-5 and worst_g[0] <= WORST_YARDSTICK


@pytest.mark.parametrize("tag", TAGS)
def test_float32_reference_run_meets_the_trajectory_criterion(tag, golden_small):
    """The criterion tests/test_gpu_sccf.py puts on three fused steps (tests/test_gpu_bigcf.py's: under 1e-3 of a table's
    elements outside rtol 1e-4 / atol 1e-6, none further than 1e-4) is one the reference's own float32 run satisfies."""
    g, gs = np.load(FIXTURE, allow_pickle=False), golden_small
    U = int(gs["num_users"])
    t, layers, lr = _setting(g, tag)
    A = _operator(tag, gs)
    W = torch.from_numpy(np.concatenate([g["init_user_embedding"], g["init_item_embedding"]]))
    tri = torch.from_numpy(g["traj_batches"])
    M, V = torch.zeros_like(W), torch.zeros_like(W)
    for i in range(3):
        bt = tri[i * 256:(i + 1) * 256]
        losses, grad, _ = ref.step64(A, W, bt[:, 0], bt[:, 1], layers, t, U, dtype=torch.float32)
        np.testing.assert_allclose(losses.numpy(), g[tag + "_traj_loss"][i], rtol=1e-5)
        step = i + 1
        M, V = 0.9 * M + 0.1 * grad, 0.999 * V + 0.001 * grad * grad
        W = W - (lr / (1 - 0.9 ** step)) * (M / (V.sqrt() / (1 - 0.999 ** step) ** 0.5 + 1e-8))
    want = np.concatenate([g[tag + "_traj_user_embedding"], g[tag + "_traj_item_embedding"]])
    off = ~np.isclose(W.numpy(), want, rtol=1e-4, atol=1e-6)
    print("%s: float32 trajectory: %.2e of the elements outside the band, at most %.2e off" % (tag, off.mean(), np.abs(W.numpy() - want).max()))
    assert off.mean() < 1e-3 and np.abs(W.numpy() - want).max() < 1e-4


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_has_every_key_the_plugin_reads():
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "SCCF.txt"), "SCCF")
    assert dict(cfg) == KEYS
    src = open(os.path.join(ROOT, "models", "SCCF.py")).read() + open(os.path.join(ROOT, "id-grec_amd", "modeling.py")).read()
    read = set(re.findall(r"config\[['\"](\w+)['\"]\]", src))
    assert {"embedding_size", "GCN_layer", "reg_lambda", "temperature", "encoder"} <= read
    assert read <= set(KEYS), read - set(KEYS)
    common = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    assert set(common) <= set(KEYS)  # the common keys of configure/LightGCN.txt are all there


def test_plugin_resolves():
    mod = importlib.import_module("models.SCCF")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.SCCF
    assert cls.supports_fused_step and cls.n_fused_losses == 2 and cls.include_layer0 is True
    for name in ("engine", "aggregate", "forward", "get_rating_for_test", "fused_step_available", "fused_train_step"):
        assert callable(getattr(cls, name)), name
    from idgrec_amd import ops
    from idgrec_amd.engine import PropagationEngine

    assert callable(ops.sccf_loss) and callable(ops.sccf_loss_raw) and callable(ops.sccf_workspace)
    assert "self.sccf = None" in open(os.path.join(ROOT, "id-grec_amd", "engine.py")).read() and PropagationEngine is not None


def test_main_names_sccf_as_implemented():
    main = open(os.path.join(ROOT, "main.py")).read()
    assert "SCCF" in re.split(r"[,.\s]+", main.split("Implemented:")[1].split("\n")[0])
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "SCCF" in [ln for ln in readme.split("\n") if "python main.py --model=" in ln][0]


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_sccf_workspace_bytes", 2), ("idg_sccf_loss_f32", 16))


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1)) == 142
    for name, n_args in ENTRY_POINTS:
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        params = re.sub(r"/\*.*?\*/", "", proto.group(1))  # (the prototype's inline comments hold commas)
        assert len(params.split(",")) == n_args == len(native.PROTOTYPES[name][1]), name
        assert hasattr(native.lib, name)
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_sccf.hip"' in build.split("SOURCES")[1].split("]")[0]
    L = native.lib
    assert 0 < L.idg_sccf_workspace_bytes(2048, 64) < (64 << 20) and L.idg_sccf_workspace_bytes(2048, 64) % 256 == 0
    assert 0 < L.idg_sccf_workspace_bytes(1, 1) and 0 < L.idg_sccf_workspace_bytes(257, 256)
    for B, d in ((0, 64), (-1, 64), (96, 0), (96, 257), (1 << 22, 64)):
        assert L.idg_sccf_workspace_bytes(B, d) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry point can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    P0, U0, I0, L0, G0, E0, WS0 = tuple(0x100000 * i for i in range(1, 7)) + (0x4000000,)

    def call(panel=P0, n=550, d=64, users=U0, pos=I0, B=96, U=300, t=0.1, loss=L0, g=G0, ge=None, acc=0, ws=WS0):
        return L.idg_sccf_loss_f32(panel, n, d, users, pos, B, U, t, loss, None, g, ge, acc, None, ws, None)

    cases = ((dict(panel=None), "NULL"), (dict(users=None), "NULL"), (dict(pos=None), "NULL"), (dict(loss=None), "NULL"),
             (dict(ws=None), "NULL"), (dict(B=0), "B = 0"), (dict(B=1 << 22), "B ="), (dict(d=0), "d = 0"), (dict(d=257), "d = 257"),
             (dict(U=0), "bad panel"), (dict(U=550), "bad panel"), (dict(t=0.0), "temperature"), (dict(t=-1.0), "temperature"),
             (dict(t=float("nan")), "temperature"), (dict(ge=G0), "distinct"), (dict(g=None, ge=E0), "distinct"),
             (dict(g=P0), "overlap"), (dict(ge=P0 + 4), "overlap"), (dict(ws=WS0 + 128), "aligned"))
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_sccf_loss_f32" in msg and word in msg, (kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    X = torch.zeros(10, 64)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.sccf_loss(X, ids, ids, 5, 0.1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.sccf_loss_raw(X, ids, ids, 5, 0.1)
    with pytest.raises(ValueError, match="not built"):
        ops.sccf_workspace(96, 300, "cpu")
