"""CGCL, host side: the fixture regenerates from the reference, the settings file carries the reference's keys, the plugin
resolves and refuses a CPU device, header / binding / library agree on the new entry points, and the wrapper's argument
checks that need no device."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cgcl_small.npz")
REF = os.environ.get("IDG_REFERENCE", "/root/reference")


def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_cgcl.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import golden_io
    finally:
        sys.path.pop(0)
    assert golden_io.same_arrays(FIXTURE, str(tmp_path / "cgcl_small.npz")) == []


def test_fixture_holds_both_settings():
    g = np.load(FIXTURE)
    for tag in ("def", "strong"):
        assert g[tag + "_loss"].shape == (5,) and g[tag + "_traj_loss"].shape == (3, 5)
        assert g[tag + "_grad_user"].shape == g[tag + "_traj_user"].shape
        assert g[tag + "_rating"].shape[0] == 32
    # the strong setting is the one where the contrastive terms carry the gradient: every user row is reached
    assert (np.abs(g["strong_grad_user"]).sum(axis=1) > 0).all()
    assert g["strong_loss"][2:].min() > 10 * g["strong_loss"][0]
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96


def test_settings_file_carries_the_reference_keys():
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "CGCL.txt"), "CGCL")
    for key in ("dataset_path", "dataset", "top_K", "training_epochs", "early_stopping", "interval", "embedding_size",
                "batch_size", "test_batch_size", "learn_rate", "reg_lambda", "GCN_layer", "ssl_lambda_alpha",
                "ssl_lambda_beta", "ssl_lambda_gamma", "alpha", "beta", "gamma", "temperature", "sparsity_test"):
        assert key in cfg, key
    assert int(cfg["batch_size"]) == 2048 and int(cfg["GCN_layer"]) == 3 and float(cfg["temperature"]) == 0.1
    assert [float(cfg[k]) for k in ("ssl_lambda_alpha", "ssl_lambda_beta", "ssl_lambda_gamma")] == [1e-5] * 3
    assert [float(cfg[k]) for k in ("alpha", "beta", "gamma")] == [0.5] * 3
    if os.path.isdir(os.path.join(REF, "configure")):
        ref = tools.read_configuration(os.path.join(REF, "configure", "CGCL.txt"), "CGCL")
        assert dict(ref) == dict(cfg)


def test_plugin_resolves_and_refuses_a_cpu_device(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    mod = importlib.import_module("models.CGCL")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    assert mod.CGCL.supports_fused_step and mod.CGCL.n_fused_losses == 5
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_train_step", "fused_loss_and_grad"):
        assert callable(getattr(mod.CGCL, name))
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "CGCL.txt"), "CGCL")
    cfg.update(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="CGCL needs an MI355X"):
        mod.CGCL(cfg, data, torch.device("cpu"))
    cfg["GCN_layer"] = "1"
    with pytest.raises(ValueError, match="GCN_layer >= 2"):
        mod.CGCL(cfg, data, torch.device("cpu"))
    assert "CGCL" in open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0]


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1))
    for name, n_args in (("idg_table_nce_workspace_bytes", 4), ("idg_table_nce_f32", 17)):
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(native.PROTOTYPES[name][1])
        assert hasattr(native.lib, name)
    assert int(re.search(r"#define IDG_TNCE_MAX_QUERY_BLOCKS (\d+)", hdr).group(1)) == native.IDG_TNCE_MAX_QUERY_BLOCKS
    # O((N + chunks nq B) d), never B x N: a quarter of one [B, N] fp32 matrix is not reached at yelp2018 shape
    ws = native.lib.idg_table_nce_workspace_bytes(2048, 38048, 64, 2)
    assert 0 < ws < 2048 * 38048 * 4 // 4
    # sizes that are not built report 0 bytes
    for B, N, d, nq in ((0, 10, 64, 1), (8, 0, 64, 1), (8, 10, 0, 1), (8, 10, 257, 1), (8, 10, 64, 0),
                        (8, 10, 64, native.IDG_TNCE_MAX_QUERY_BLOCKS + 1)):
        assert native.lib.idg_table_nce_workspace_bytes(B, N, d, nq) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for arguments the entry point can judge on the host."""
    import ctypes as C

    from idgrec_amd import native

    one = (C.c_void_p * 1)(8)
    w = (C.c_float * 1)(1.0)

    def call(table=8, N=10, d=64, nq=1, B=4, pos=8, tau=0.1, loss=8, g_table=None, g_q=None, ws=256):
        return native.lib.idg_table_nce_f32(table, 0, N, d, nq, one, one, B, pos, w, tau, loss, None, g_table, g_q, ws, None)

    for kw, word in ((dict(table=None), "NULL"), (dict(pos=None), "NULL"), (dict(ws=None), "NULL"), (dict(B=0), "bad sizes"),
                     (dict(N=0), "bad sizes"), (dict(d=257), "d = 257"), (dict(nq=0), "nq = 0"), (dict(nq=5), "nq = 5"),
                     (dict(tau=0.0), "temperature"), (dict(tau=-1.0), "temperature"), (dict(loss=None), "nothing to compute"),
                     (dict(g_table=8), "go together"), (dict(table=6), "misaligned"), (dict(ws=264), "misaligned")):
        assert call(**kw) == -1, kw
        assert word in native.lib.idg_last_error().decode(), (kw, native.lib.idg_last_error())


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    t = torch.zeros(10, 8)
    ids = torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.table_nce_raw(t, 0, 10, [t], [ids], ids, [1.0], 0.1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.table_nce_loss(t, 0, 10, [t], [ids], ids, [1.0], 0.1)
    with pytest.raises(ValueError, match="temperature"):
        ops.table_nce_raw(t, 0, 10, [t], [ids], ids, [1.0], 0.0)
    with pytest.raises(ValueError, match="query blocks"):
        ops.table_nce_raw(t, 0, 10, [t] * 5, [ids] * 5, ids, [1.0] * 5, 0.1)
    with pytest.raises(ValueError, match="query blocks"):
        ops.table_nce_raw(t, 0, 10, [], [], ids, [], 0.1)
    with pytest.raises(ValueError, match="weights"):
        ops.table_nce_raw(t, 0, 10, [t], [ids], ids, [1.0, 2.0], 0.1)
    with pytest.raises(ValueError, match="not inside"):
        ops.table_nce_loss(t, 2, 10, [t], [ids], ids, [1.0], 0.1)
    with pytest.raises(ValueError, match="query panel 0"):
        ops.table_nce_raw(t, 0, 10, [torch.zeros(10, 9)], [ids], ids, [1.0], 0.1)
    with pytest.raises(ValueError, match="id list 0"):
        ops.table_nce_raw(t, 0, 10, [t], [ids[:3]], ids, [1.0], 0.1)
    with pytest.raises(ValueError, match="width 300"):
        ops.table_nce_raw(torch.zeros(10, 300), 0, 10, [torch.zeros(10, 300)], [ids], ids, [1.0], 0.1)
    with pytest.raises(ValueError, match="go together"):
        ops.table_nce_raw(t, 0, 10, [t], [ids], ids, [1.0], 0.1, g_table=torch.zeros_like(t))
