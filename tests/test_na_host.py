"""LightCCF / LightCSCF, host side: the fixture regenerates from the reference and holds its four settings;
tests/na_ref64.py — the float64 statement tests/test_gpu_na.py holds the kernels against — reproduces the reference's
losses, both gradients and the rating in its literal (two matmuls added) and its collapsed (A (A + B)^T) form, and the two
forms agree, also on edge batches; every LightCSCF case keeps its scores away from the margin's kink; the float32 yardstick
of the GPU tests is measured and printed; the reference's own float32 run meets the trajectory criterion; the settings files
carry every key the plugins read; header / binding / library agree on the entry points of csrc/idg_nance.hip, and their
argument checks come before any device work.

The fixture is the reference's own program run in float64 from its float32 initial tables (scripts/gen_golden_na.py), so the
statement is held to it at 1e-10 — the losses, stored as float64, directly; the gradients and ratings, stored rounded to
float32, after the same rounding.  Measured here: losses equal to 4e-16, the float32-rounded arrays identical or one
float32 step apart where the float64 value sits on a rounding boundary (at most 6e-8 of the largest entry); the two forms
agree to 3e-16 (losses) and 2e-14 (gradients).
The float32 yardstick (the literal form in float32 against the float64 statement; losses relative, gradients as a share of
the largest float64 entry) is recorded by test_float32_yardstick_is_measured's printout; its worst gradient case sets
tests/test_gpu_na.py's GRAD_TOL (twice it, capped by the siblings' 1e-5) — see GRAD_CAP below.  The reference's own float32
run on the fixture's three batches: `ccf_mf` no element outside rtol 1e-4 / atol 1e-6 (1.4e-6 off at most); the other three
settings are printed by test_float32_reference_run_meets_the_trajectory_criterion (LightCCF on LightGCN at T = 0.1 does NOT
meet it — near-zero gradient elements change sign in float32 and Adam turns the sign into a full step — which is why the
fixture's `ccf_gcn` runs at T = 0.15)."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import na_ref64 as ref  # noqa: E402
from tests import widths  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "na_small.npz")
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
KEYS_CCF = dict(dataset_path="./dataset/", dataset="amazon-book", top_K="[10, 20]", training_epochs="50", early_stopping="20",
                interval="1", embedding_size="64", batch_size="4096", test_batch_size="200", learn_rate="0.001",
                reg_lambda="0.0001", GCN_layer="3", ssl_lambda="5.0", temperature="0.22", encoder="LightGCN", sparsity_test="0")
KEYS_CSCF = dict(dataset_path="./dataset/", dataset="amazon-book", top_K="[10, 20]", training_epochs="1000", early_stopping="20",
                 interval="1", embedding_size="64", batch_size="4096", test_batch_size="4096", learn_rate="0.001",
                 lambda_reg="0.0001", GCN_layer="3", lambda_gamma="1.0", lambda_margin="0.7", temperature="0.2",
                 encoder="LightGCN", sparsity_test="0")
TAGS = tuple(ref.SETTINGS)
PARAMS = ("user_embedding", "item_embedding")
# The worst float32 yardstick of the gradients this file measures (test_float32_yardstick_is_measured prints every figure):
# 3.2e-2 of the largest entry — LightCCF at T = 0.05, B = 129, d = 64: the gradient there is the 1e5 times smaller rest of
# parts that cancel (the diagonal and the columns repeating the row's user hold nearly all of every row sum), and float32
# rounds the parts.  Next: one user repeated 96 times, LightCCF, T = 0.1: 1.8e-5; one user 257 times with the margin: 8.4e-6;
# the LightCCF cases of the grid at T = 0.1: 1.6e-6 ... 4.5e-6; every case at T = 1 and every other LightCSCF case: under 2.4e-6.
# tests/test_gpu_na.py's GRAD_TOL is twice the worst figure capped by the siblings' 1e-5.  Twice the worst is far above the
# cap, so the cap holds — as long as the measurement stays above half of it, which the test asserts.
GRAD_CAP = 1e-5


def _init(g, tag):
    d = int(g[tag + "_hyper"][6])
    return torch.from_numpy(np.concatenate([g["init%d_user_embedding" % d], g["init%d_item_embedding" % d]]))


def _operator(tag, gs):
    n = int(gs["num_users"]) + int(gs["num_items"])
    if ref.SETTINGS[tag][1] == "MF":
        return None
    return ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (n, n))


def _step(g, gs, tag, W, bt, **kw):
    reg, weight, margin, with_bpr, t, layers, _ = ref.setting_terms(tag, g[tag + "_hyper"][:6])
    return ref.step64(_operator(tag, gs), W, bt[:, 0], bt[:, 1], bt[:, 2], layers, t, int(gs["num_users"]), reg, weight, margin,
                      with_bpr, **kw)


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_na.py")], check=True, env=env, cwd=ROOT,
                   stdout=subprocess.DEVNULL)
    assert open(FIXTURE, "rb").read() == open(str(tmp_path / "na_small.npz"), "rb").read()


def test_fixture_holds_the_four_settings():
    assert os.path.getsize(FIXTURE) <= (1 << 20)
    g = np.load(FIXTURE, allow_pickle=False)
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert b[9, 2] == b[9, 1] and b[11, 2] == b[10, 2]  # a negative equal to a positive, a repeated negative
    assert g["traj_batches"].shape == (768, 3) and g["rating_users"].shape == (32,)
    want = {"ccf_mf": (0.22, 3, 1e-3, 1e-4, 5.0, -1.0, 64), "ccf_gcn": (0.15, 2, 1e-3, 0.01, 5.0, -1.0, 64),
            "cscf_mf": (0.2, 3, 1e-3, 1e-4, 1.0, 0.7, 32), "cscf_gcn": (0.2, 3, 1e-3, 0.05, 2.0, 0.5, 32)}
    for tag in TAGS:
        assert tuple(g[tag + "_hyper"].tolist()) == want[tag]
        nl = 2 if tag == "cscf_gcn" else 3
        d = int(g[tag + "_hyper"][6])
        assert g[tag + "_loss"].shape == (nl,) and g[tag + "_traj_loss"].shape == (3, nl) and g[tag + "_rating"].shape == (32, 250)
        assert g[tag + "_loss"].dtype == np.float64 and np.isfinite(g[tag + "_loss"]).all() and np.isfinite(g[tag + "_traj_loss"]).all()
        for p, rows in zip(PARAMS, (300, 250)):
            assert g["init%d_%s" % (d, p)].shape == (rows, d)
            for pre in ("grad", "traj"):
                a = g["%s_%s_%s" % (tag, pre, p)]
                assert a.shape == (rows, d) and a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
            moved = np.abs(g["%s_traj_%s" % (tag, p)] - g["init%d_%s" % (d, p)]).max()
            assert 1e-4 < moved <= 3.01e-3  # three Adam steps at lr = 1e-3


# ------------------------------------------------------------------------------- the float64 statement is the reference's
@pytest.mark.parametrize("tag", TAGS)
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, gs = np.load(FIXTURE, allow_pickle=False), golden_small
    U = int(gs["num_users"])
    E0 = _init(g, tag)
    b = torch.from_numpy(g["batch"])
    want = np.concatenate([g[tag + "_grad_user_embedding"], g[tag + "_grad_item_embedding"]])
    margin = ref.setting_terms(tag, g[tag + "_hyper"][:6])[2]
    res = {}
    for collapsed in (False, True):
        losses, gE0, X = _step(g, gs, tag, E0, b, collapsed=collapsed)
        assert losses.dtype == gE0.dtype == X.dtype == torch.float64 and losses.shape == g[tag + "_loss"].shape
        if margin is not None:
            assert ref.kink_distance(X, U, b[:, 0], b[:, 1], margin) > ref.KINK_GAP
        e_loss = float(np.abs(losses.numpy() / g[tag + "_loss"] - 1).max())
        # the fixture stores float32: round the statement the same way, and allow the one float32 step of a float64 value
        # that sits on a rounding boundary (the 1e-10 is on the float64 values: 1e-10 relative moves the rounding of 1e-3 of them)
        mine = gE0.numpy().astype(np.float32)
        e_grad = float(np.abs(mine.astype(np.float64) - want).max() / np.abs(want).max())
        near = np.abs(gE0.numpy() - want) <= np.abs(gE0.numpy()) * 1e-10 + np.spacing(np.abs(want)) * 0.5000001
        print("%s (%s): losses %.2e (relative); gradients rounded to float32 %.2e of the largest entry from the fixture, %d of "
              "%d elements not identical" % (tag, "collapsed" if collapsed else "literal", e_loss, e_grad, int((mine != want).sum()), want.size))
        np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=1e-10)
        assert bool(near.all())
        users = torch.from_numpy(g["rating_users"])
        rating = torch.sigmoid(X[users] @ X[U:].t()).numpy()
        assert bool((np.abs(rating - g[tag + "_rating"]) <= rating * 1e-10 + np.spacing(g[tag + "_rating"]) * 0.5000001).all())
        res[collapsed] = (losses, gE0)
    (l_l, g_l), (l_c, g_c) = res[False], res[True]
    e_l, e_g = float(((l_c - l_l) / l_l).abs().max()), float((g_c - g_l).abs().max() / g_l.abs().max())
    print("%s: collapsed against literal: losses %.2e, gradients %.2e" % (tag, e_l, e_g))
    assert e_l <= 1e-12 and e_g <= 1e-12


@pytest.mark.parametrize("margin", ref.GRID_M)
@pytest.mark.parametrize("form,B", [("random", 1), ("distinct", 37), ("distinct", 96), ("one_user", 37), ("one_user", 96),
                                    ("zero_rows", 37)])
def test_the_two_forms_agree_on_edge_batches(form, B, margin):
    """B = 1, all ids distinct, one user repeated B times, a zero panel row as a user and as a positive."""
    for d, t in ((24, 0.1), (64, 1.0)):
        panel, users, pos, U = ref.case_inputs(B, d, 11 + B, form=form)
        if form in ("distinct", "one_user"):
            assert int(torch.unique(users).numel()) == (B if form == "distinct" else 1)
        if margin is not None:
            assert ref.kink_distance(panel, U, users, pos, margin) > ref.KINK_GAP
        l_l, g_l = ref.panel_terms(panel, U, users, pos, t, margin)
        l_c, g_c = ref.panel_terms(panel, U, users, pos, t, margin, collapsed=True)
        assert bool(torch.isfinite(l_l)) and bool(torch.isfinite(g_l).all())
        assert float(((l_c - l_l) / l_l).abs()) <= 1e-12
        assert float((g_c - g_l).abs().max()) <= 1e-12 * ref.grad_scale(panel, U, users, pos, t, margin, g_l)


def test_every_lightcscf_case_keeps_away_from_the_margin():
    """relu(s - m) has a kink at m: float32 and float64 must take the same branch, so no score (and no positive) of a case
    with a margin lies within KINK_GAP of it.  The seeds of tests/na_ref64.py were chosen so; none is skipped."""
    worst = 1.0
    for form, B, d, t, m, seed in ref.all_cases():
        if m is None:
            continue
        panel, users, pos, U = ref.case_inputs(B, d, seed, form=form)
        gap = ref.kink_distance(panel, U, users, pos, m)
        worst = min(worst, gap)
        assert gap > ref.KINK_GAP, (form, B, d, t, gap)
    print("smallest distance of a score from the margin over every case: %.2e" % worst)


# ------------------------------------------------------------------------------------------------- the float32 yardstick
def test_float32_yardstick_is_measured(golden_small):
    """The largest distance of the float32 literal form from the float64 statement, over the fixture's inputs and every case
    tests/test_gpu_na.py runs (the same seeds, on the CPU).  Printed, with its worst case named."""
    g, gs = np.load(FIXTURE, allow_pickle=False), golden_small
    b = torch.from_numpy(g["batch"])
    worst_l, worst_g = (0.0, None), (0.0, None)
    for tag in TAGS:
        l64, g64, _ = _step(g, gs, tag, _init(g, tag), b)
        l32, g32, _ = _step(g, gs, tag, _init(g, tag), b, dtype=torch.float32)
        e_l, e_g = float(((l32.double() - l64) / l64).abs().max()), float((g32.double() - g64).abs().max() / g64.abs().max())
        print("fixture %s: float32 literal form: losses %.2e, gradients %.2e of the largest entry" % (tag, e_l, e_g))
        worst_l, worst_g = max(worst_l, (e_l, "fixture " + tag)), max(worst_g, (e_g, "fixture " + tag))
    for form, B, d, t, m, seed in ref.all_cases():
        panel, users, pos, U = ref.case_inputs(B, d, seed, form=form)
        up = ref.grid_upstream(B) if form == "random" and seed == ref.grid_seed(B, d, t) else None
        l64, g64 = ref.panel_terms(panel, U, users, pos, t, m, upstream=up)
        l32, g32 = ref.panel_terms(panel, U, users, pos, t, m, dtype=torch.float32, upstream=up)
        keep = torch.ones(panel.shape[0], dtype=torch.bool)
        if form == "zero_rows":
            keep[list(ref.zero_rows_of(users, pos, U))] = False
        e_l = float(((l32.double() - l64) / l64).abs())
        e_g = float((g32.double() - g64)[keep].abs().max()) / ref.grad_scale(panel, U, users, pos, t, m, g64[keep], upstream=up)
        name = "%s B=%d d=%d T=%g margin=%s" % (form, B, d, t, m)
        if form != "random" or e_g > 1e-6:
            print("%s: losses %.2e, gradients %.2e of the largest entry" % (name, e_l, e_g))
        worst_l, worst_g = max(worst_l, (e_l, name)), max(worst_g, (e_g, name))
    print("float32 yardstick: losses %.2e (%s); gradients %.2e of the largest entry (%s)" % (worst_l + worst_g))
    assert worst_l[0] < 1e-5
    assert 2 * worst_g[0] >= GRAD_CAP  # the bound of tests/test_gpu_na.py is min(2 * yardstick, cap) = the cap


def test_every_built_width_case_is_away_from_the_margin_and_its_yardstick_is_measured():
    """The cases tests/test_gpu_na.py runs over tests/widths.py's EVERY_NDT (the same seeds, on the CPU): every LightCSCF case
    keeps KINK_GAP from the margin, and the float32 yardstick of each is printed.  Twice the worst of them (4.3e-6: LightCCF,
    B = 257, d = 224) stays under GRAD_CAP, so these cases take tests/test_gpu_na.py's GRAD_TOL = GRAD_CAP unchanged."""
    worst_l, worst_g, gap_min = (0.0, None), (0.0, None), 1.0
    seeds = set()
    for form, B, d, t, m, seed in ref.width_cases(widths.EVERY_NDT):
        seeds.add(seed)
        panel, users, pos, U = ref.case_inputs(B, d, seed, form=form)
        if m is not None:
            gap = ref.kink_distance(panel, U, users, pos, m)
            gap_min = min(gap_min, gap)
            assert gap > ref.KINK_GAP, (B, d, gap)
        up = ref.grid_upstream(B)
        l64, g64 = ref.panel_terms(panel, U, users, pos, t, m, upstream=up)
        l32, g32 = ref.panel_terms(panel, U, users, pos, t, m, dtype=torch.float32, upstream=up)
        e_l = float(((l32.double() - l64) / l64).abs())
        e_g = float((g32.double() - g64).abs().max()) / ref.grad_scale(panel, U, users, pos, t, m, g64, upstream=up)
        name = "widths B=%d d=%d T=%g margin=%s" % (B, d, t, m)
        print("%s: losses %.2e, gradients %.2e of the largest entry" % (name, e_l, e_g))
        worst_l, worst_g = max(worst_l, (e_l, name)), max(worst_g, (e_g, name))
    print("every built width: losses %.2e (%s); gradients %.2e of the largest entry (%s); smallest distance from the margin %.2e"
          % (worst_l + worst_g + (gap_min,)))
    assert worst_l[0] < 1e-5 and 2 * worst_g[0] <= GRAD_CAP
    assert not seeds & {s for c in ref.all_cases() for s in c[5:]}  # no seed of the older cases is drawn again


@pytest.mark.parametrize("tag", TAGS)
def test_float32_reference_run_meets_the_trajectory_criterion(tag, golden_small):
    """The criterion tests/test_gpu_na.py puts on three fused steps (tests/test_gpu_bigcf.py's: under 1e-3 of a table's
    elements outside rtol 1e-4 / atol 1e-6, none further than 1e-4) is one the reference's own float32 run satisfies."""
    g, gs = np.load(FIXTURE, allow_pickle=False), golden_small
    lr = float(g[tag + "_hyper"][2])
    W = _init(g, tag)
    tri = torch.from_numpy(g["traj_batches"])
    M, V = torch.zeros_like(W), torch.zeros_like(W)
    for i in range(3):
        bt = tri[i * 256:(i + 1) * 256]
        losses, grad, _ = _step(g, gs, tag, W, bt, dtype=torch.float32)
        np.testing.assert_allclose(losses.numpy(), g[tag + "_traj_loss"][i], rtol=1e-5)
        step = i + 1
        M, V = 0.9 * M + 0.1 * grad, 0.999 * V + 0.001 * grad * grad
        W = W - (lr / (1 - 0.9 ** step)) * (M / (V.sqrt() / (1 - 0.999 ** step) ** 0.5 + 1e-8))
    want = np.concatenate([g[tag + "_traj_user_embedding"], g[tag + "_traj_item_embedding"]])
    off = ~np.isclose(W.numpy(), want, rtol=1e-4, atol=1e-6)
    print("%s: float32 trajectory: %.2e of the elements outside the band, at most %.2e off" % (tag, off.mean(), np.abs(W.numpy() - want).max()))
    assert off.mean() < 1e-3 and np.abs(W.numpy() - want).max() < 1e-4


# ------------------------------------------------------------------------------------------ settings, plugins, main.py
@pytest.mark.parametrize("name,keys,own", [("LightCCF", KEYS_CCF, {"reg_lambda", "ssl_lambda", "temperature", "encoder"}),
                                           ("LightCSCF", KEYS_CSCF, {"lambda_reg", "lambda_gamma", "lambda_margin", "temperature", "encoder"})])
def test_settings_files_have_every_key_the_plugins_read(name, keys, own):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", name + ".txt"), name)
    assert dict(cfg) == keys
    src = "".join(open(os.path.join(ROOT, *p)).read() for p in (("models", name + ".py"), ("models", "LightCCF.py"),
                                                                ("id-grec_amd", "modeling.py")))
    read = set(re.findall(r"config\[['\"](\w+)['\"]\]", src))
    assert own | {"GCN_layer", "embedding_size"} <= read
    # LightCSCF hands its two weights to the shared base under LightCCF's names; every other key read is in its own file
    assert read - ({"reg_lambda", "ssl_lambda"} if name == "LightCSCF" else set()) <= set(keys), read - set(keys)
    common = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    assert set(common) - {"reg_lambda"} <= set(keys)  # the common keys of configure/LightGCN.txt are all there


def test_plugins_resolve():
    for name, nl in (("LightCCF", 3), ("LightCSCF", 3)):
        mod = importlib.import_module("models." + name)
        assert callable(mod.Trainer) and callable(mod.Trainer.train)
        cls = getattr(mod, name)
        assert cls.supports_fused_step and cls.n_fused_losses == nl and cls.include_layer0 is True
        for fn in ("engine", "aggregate", "forward", "get_rating_for_test", "fused_step_available", "fused_train_step"):
            assert callable(getattr(cls, fn)), fn
    src = open(os.path.join(ROOT, "models", "LightCSCF.py")).read()
    assert "self.n_fused_losses = 3 if self.with_bpr else 2" in src  # [reg, na] on a non-MF encoder
    from idgrec_amd import ops
    from idgrec_amd.engine import PropagationEngine

    for fn in ("na_nce_loss", "na_nce_loss_raw", "na_nce_workspace", "reg_rows_raw", "reg_rows_loss"):
        assert callable(getattr(ops, fn)), fn
    eng = open(os.path.join(ROOT, "id-grec_amd", "engine.py")).read()
    assert "self.na = None" in eng and "self.na is None" in eng.split("def _plan_eligible")[1].split("def ")[0]
    assert PropagationEngine is not None


def test_main_names_both_plugins_as_implemented():
    main = open(os.path.join(ROOT, "main.py")).read()
    named = re.split(r"[,.\s]+", main.split("Implemented:")[1].split("\n")[0])
    assert "LightCCF" in named and "LightCSCF" in named
    readme = open(os.path.join(ROOT, "README.md")).read()
    line = [ln for ln in readme.split("\n") if "python main.py --model=" in ln][0]
    assert "LightCCF" in line and "LightCSCF" in line


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_na_nce_workspace_bytes", 2), ("idg_na_nce_f32", 17), ("idg_reg_rows_f32", 15))


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1))
    for name, n_args in ENTRY_POINTS:
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        params = re.sub(r"/\*.*?\*/", "", proto.group(1))  # (the prototype's inline comments hold commas)
        assert len(params.split(",")) == n_args == len(native.PROTOTYPES[name][1]), name
        assert hasattr(native.lib, name)
        assert name in hdr.split("#define IDG_VERSION")[1].split("\n")[0] or name == "idg_na_nce_workspace_bytes"  # named as additive
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_nance.hip"' in build.split("SOURCES")[1].split("]")[0]
    L = native.lib
    assert 0 < L.idg_na_nce_workspace_bytes(4096, 64) < (160 << 20) and L.idg_na_nce_workspace_bytes(4096, 64) % 256 == 0
    assert 0 < L.idg_na_nce_workspace_bytes(1, 1) and 0 < L.idg_na_nce_workspace_bytes(257, 256)
    for B, d in ((0, 64), (-1, 64), (96, 0), (96, 257), (1 << 22, 64)):
        assert L.idg_na_nce_workspace_bytes(B, d) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    P0, U0, I0, L0, G0, E0, WS0 = tuple(0x100000 * i for i in range(1, 7)) + (0x4000000,)

    def call(panel=P0, n=550, d=64, users=U0, pos=I0, B=96, U=300, t=0.1, m=-1.0, w=1.0, loss=L0, g=G0, acc=0, ws=WS0):
        return L.idg_na_nce_f32(panel, n, d, users, pos, B, U, t, m, w, loss, None, g, acc, None, ws, None)

    cases = ((dict(panel=None), "NULL"), (dict(users=None), "NULL"), (dict(pos=None), "NULL"), (dict(loss=None), "NULL"),
             (dict(ws=None), "NULL"), (dict(B=0), "B = 0"), (dict(B=1 << 22), "B ="), (dict(d=0), "d = 0"), (dict(d=257), "d = 257"),
             (dict(U=0), "bad panel"), (dict(U=550), "bad panel"), (dict(t=0.0), "temperature"), (dict(t=-1.0), "temperature"),
             (dict(t=0.005), "temperature"), (dict(t=float("nan")), "temperature"), (dict(m=2.5), "margin"),
             (dict(m=float("nan")), "margin"), (dict(w=float("inf")), "grad_scale"), (dict(g=P0), "overlap"),
             (dict(g=P0 + 4), "overlap"), (dict(ws=WS0 + 128), "aligned"))
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_na_nce_f32" in msg and word in msg, (kw, msg)

    def reg(panel=P0, n=550, d=64, users=U0, pos=I0, neg=I0 + 0x1000, B=96, U=300, lam=1e-4, loss=L0, ge=E0, g=G0, plan=None, ws=WS0):
        return L.idg_reg_rows_f32(panel, n, d, users, pos, neg, B, U, lam, loss, ge, g, plan, ws, None)

    cases = ((dict(panel=None), "NULL"), (dict(loss=None), "NULL"), (dict(ws=None), "NULL"), (dict(neg=None), "id lists"),
             (dict(users=None), "id lists"), (dict(B=0), "B = 0"), (dict(d=257), "d = 257"), (dict(U=550), "bad panel"),
             (dict(lam=float("nan")), "reg_lambda"), (dict(g=E0), "distinct"), (dict(ge=P0), "overlap"), (dict(g=P0 + 4), "overlap"),
             (dict(g=E0 + 4), "overlap"), (dict(ws=WS0 + 128), "aligned"))
    for kw, word in cases:
        assert reg(**kw) == -1, kw
        msg = L.idg_last_error().decode()
        assert "idg_reg_rows_f32" in msg and word in msg, (kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    X = torch.zeros(10, 64)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.na_nce_loss(X, ids, ids, 5, 0.1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.na_nce_loss_raw(X, ids, ids, 5, 0.1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.reg_rows_raw(X, ids, ids, ids, 5, 1e-4)
    with pytest.raises(ValueError, match="not built"):
        ops.na_nce_workspace(96, 300, "cpu")
