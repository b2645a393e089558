"""DirectAU, host side: the fixture regenerates from the reference, the torch loss functions under the reference's names
match it (the one-row NaN included), the settings file and the plugin resolve."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "directau_small.npz")


@pytest.fixture(scope="module")
def golden_au():
    return dict(np.load(FIXTURE))


def test_fixture_regenerates_from_the_reference(tmp_path):
    ref = os.environ.get("IDG_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "models")):
        pytest.skip("needs the reference tree (%s)" % ref)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_directau.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import golden_io
    finally:
        sys.path.pop(0)
    assert golden_io.same_arrays(FIXTURE, str(tmp_path / "directau_small.npz")) == []


@pytest.mark.parametrize("B", [1, 2])
def test_loss_functions_match_the_reference(B, golden_au):
    from utility.utility_function import losses

    g = golden_au
    x = torch.from_numpy(g["blk%d_x" % B]).requires_grad_(True)
    y = torch.from_numpy(g["blk%d_y" % B]).requires_grad_(True)
    a = losses.get_align_loss(x, y)
    a.backward()
    np.testing.assert_allclose(a.item(), g["blk%d_align" % B], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(x.grad.numpy(), g["blk%d_align_gx" % B], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(y.grad.numpy(), g["blk%d_align_gy" % B], rtol=1e-6, atol=1e-7)
    x = torch.from_numpy(g["blk%d_x" % B]).requires_grad_(True)
    u = losses.get_uniform_loss(x)
    u.backward()
    if B == 1:  # no pair: the mean of nothing, and no gradient
        assert np.isnan(g["blk1_uniform"]) and np.isnan(u.item())
        assert not x.grad.any() and not np.any(g["blk1_uniform_gx"])
    else:
        np.testing.assert_allclose(u.item(), g["blk2_uniform"], rtol=1e-6)
        np.testing.assert_allclose(x.grad.numpy(), g["blk2_uniform_gx"], rtol=1e-6, atol=1e-7)


def test_settings_file_parses_with_interval():
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "DirectAU.txt"), "DirectAU")
    assert int(cfg["interval"]) >= 1
    assert cfg["encoder"] in ("LightGCN", "MF")
    assert float(cfg["gamma"]) == 2.0 and int(cfg["batch_size"]) == 2048
    for key in ("embedding_size", "learn_rate", "reg_lambda", "GCN_layer", "top_K", "training_epochs", "early_stopping"):
        assert key in cfg


def test_plugin_resolves():
    mod = importlib.import_module("models.DirectAU")
    assert callable(mod.Trainer)
    assert mod.DirectAU.supports_fused_step and mod.DirectAU.n_fused_losses == 3
    from idgrec_amd import ops

    assert callable(ops.align_uniform_loss) and callable(ops.align_uniform_raw)
