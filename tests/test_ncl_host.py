"""NCL, host side: the fixture regenerates from the reference, the settings file carries the reference's keys, the plugin
resolves and refuses a CPU device, header / binding / library agree on the k-means entry points, and the argument checks of
the library and of the wrappers that need no device."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ncl_small.npz")
REF = os.environ.get("IDG_REFERENCE", "/root/reference")
REF_KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="500", early_stopping="20",
                interval="1", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.001",
                reg_lambda="0.0001", GCN_layer="3", ssl_lambda="1e-6", proto_lambda="1e-7", temperature="0.05", cl_layer="1",
                alpha="1.5", k="2000", sparsity_test="0")


def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_ncl.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import golden_io
    finally:
        sys.path.pop(0)
    assert golden_io.same_arrays(FIXTURE, str(tmp_path / "ncl_small.npz")) == []


def test_fixture_holds_both_settings_and_both_epochs():
    g = np.load(FIXTURE)
    for tag in ("def", "strong"):
        assert g[tag + "_loss0"].shape == (3,) and g[tag + "_loss20"].shape == (4,) and g[tag + "_traj_loss"].shape == (3, 4)
        for e in ("0", "20"):
            assert g[tag + "_grad_user" + e].shape == g[tag + "_traj_user"].shape == (300, 64)
            assert g[tag + "_grad_item" + e].shape == g[tag + "_traj_item"].shape == (250, 64)
        # the first three terms do not depend on the epoch; the prototype term changes the gradient
        assert np.array_equal(g[tag + "_loss0"], g[tag + "_loss20"][:3])
        assert not np.array_equal(g[tag + "_grad_user0"], g[tag + "_grad_user20"])
        assert g[tag + "_rating"].shape == (32, 250)
    # the strong setting is the one where the two extra terms carry the gradient: every row of both tables is reached
    assert (np.abs(g["strong_grad_user0"]).sum(axis=1) > 0).all() and (np.abs(g["strong_grad_item0"]).sum(axis=1) > 0).all()
    assert g["strong_loss20"][2:].min() > 10 * g["strong_loss20"][0]
    assert g["user_centroids"].shape == g["item_centroids"].shape == (16, 64)
    assert g["user_2cluster"].shape == (300,) and g["item_2cluster"].shape == (250,)
    for key in ("user_2cluster", "item_2cluster"):
        assert g[key].min() >= 0 and g[key].max() < 16 and len(set(g[key].tolist())) == 16
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96


def test_settings_file_carries_the_reference_keys():
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "NCL.txt"), "NCL")
    for key, value in REF_KEYS.items():
        assert cfg.get(key) == value, key
    assert (int(cfg["proto_warmup"]), int(cfg["kmeans_niter"]), int(cfg["kmeans_seed"])) == (20, 25, 1234)
    assert set(cfg) == set(REF_KEYS) | {"proto_warmup", "kmeans_niter", "kmeans_seed"}
    if os.path.isdir(os.path.join(REF, "configure")):
        ref = tools.read_configuration(os.path.join(REF, "configure", "NCL.txt"), "NCL")
        assert dict(ref) == REF_KEYS
        assert {k: cfg[k] for k in ref} == dict(ref)


def test_plugin_resolves_and_refuses_a_cpu_device(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    mod = importlib.import_module("models.NCL")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    assert mod.NCL.supports_fused_step and mod.NCL.n_fused_losses == 4 and mod.NCL.include_layer0
    for name in ("aggregate", "forward", "E_step", "begin_epoch", "get_rating_for_test", "topk_for_test", "fused_train_step",
                 "fused_loss_and_grad"):
        assert callable(getattr(mod.NCL, name))
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "NCL.txt"), "NCL")
    cfg.update(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0", k="4")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="NCL needs an MI355X"):
        mod.NCL(cfg, data, torch.device("cpu"))
    with pytest.raises(ValueError, match="GCN_layer >= 2 \\* cl_layer"):
        mod.NCL(dict(cfg, GCN_layer="1"), data, torch.device("cpu"))
    with pytest.raises(ValueError, match="GCN_layer >= 2 \\* cl_layer"):
        mod.NCL(dict(cfg, cl_layer="2"), data, torch.device("cpu"))
    with pytest.raises(ValueError, match="clusters for tables"):
        mod.NCL(dict(cfg, k=str(min(data.num_users, data.num_items) + 1)), data, torch.device("cpu"))
    assert "NCL" in open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0]
    # the trainer's hook: called once at the top of every epoch when the model has it
    src = open(os.path.join(ROOT, "utility", "utility_train", "trainer.py")).read()
    assert src.count("begin_epoch") == 1


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1))
    for name, n_args in (("idg_kmeans_workspace_bytes", 3), ("idg_kmeans_assign_f32", 10), ("idg_kmeans_update_f32", 10),
                         ("idg_kmeans_f32", 11)):
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(native.PROTOTYPES[name][1])
        assert hasattr(native.lib, name)
    # O((N + K) d + chunks N), never N x K
    ws = native.lib.idg_kmeans_workspace_bytes(38048, 2000, 64)
    assert 0 < ws < 38048 * 2000 * 4 // 4
    # sizes that are not built report 0 bytes
    for N, K, d in ((0, 10, 64), (10, 0, 64), (10, 4, 0), (10, 4, 257), (1 << 31, 4, 64), (10, 1 << 31, 64), (-1, 4, 64)):
        assert native.lib.idg_kmeans_workspace_bytes(N, K, d) == 0, (N, K, d)
    assert native.lib.idg_kmeans_workspace_bytes(1, 1, 1) > 0 and native.lib.idg_kmeans_workspace_bytes(10, 4, 256) > 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for arguments the entry points can judge on the host."""
    from idgrec_amd import native

    L = native.lib

    def assign(X=8, ldx=64, N=10, d=64, C=8, K=4, a=8, dist2=None, ws=256):
        return L.idg_kmeans_assign_f32(X, ldx, N, d, C, K, a, dist2, ws, None)

    def update(X=8, ldx=64, N=10, d=64, a=8, K=4, C=8, counts=None, ws=256):
        return L.idg_kmeans_update_f32(X, ldx, N, d, a, K, C, counts, ws, None)

    def full(X=8, ldx=64, N=10, d=64, K=4, niter=3, C=8, a=8, inertia=None, ws=256):
        return L.idg_kmeans_f32(X, ldx, N, d, K, niter, C, a, inertia, ws, None)

    common = ((dict(X=None), "NULL"), (dict(C=None), "NULL"), (dict(a=None), "NULL"), (dict(ws=None), "NULL"),
              (dict(N=0), "bad sizes"), (dict(K=0), "bad sizes"), (dict(K=-3), "bad sizes"), (dict(d=0, ldx=0), "d = 0"),
              (dict(d=257, ldx=257), "d = 257"), (dict(ldx=63), "ldx = 63"), (dict(N=1 << 31), "int32"),
              (dict(K=1 << 31), "int32"), (dict(X=6), "misaligned"), (dict(ws=264), "misaligned"))
    for fn, who in ((assign, "idg_kmeans_assign_f32"), (update, "idg_kmeans_update_f32"), (full, "idg_kmeans_f32")):
        for kw, word in common:
            assert fn(**kw) == -1, (who, kw)
            msg = L.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)
    assert full(niter=-1) == -1 and "niter = -1" in L.idg_last_error().decode()


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    X = torch.zeros(10, 8)
    C = torch.zeros(4, 8)
    a = torch.zeros(10, dtype=torch.int32)
    # host tensors
    for call in (lambda: ops.kmeans(X, 4), lambda: ops.kmeans_assign_raw(X, C), lambda: ops.kmeans_update_raw(X, a, C),
                 lambda: ops.kmeans_raw(X, C, 3)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    # more clusters than rows, no clusters
    with pytest.raises(ValueError, match="K = 11 clusters for N = 10 rows"):
        ops.kmeans(X, 11)
    with pytest.raises(ValueError, match="K = 0 clusters"):
        ops.kmeans(X, 0)
    # wrong dtypes and shapes
    with pytest.raises(TypeError, match="float32"):
        ops.kmeans(X.double(), 4)
    with pytest.raises(TypeError, match="float32"):
        ops.kmeans_assign_raw(X.double(), C)
    with pytest.raises(TypeError, match="centroids"):
        ops.kmeans_assign_raw(X, C.double())
    with pytest.raises(TypeError, match="centroids"):
        ops.kmeans_assign_raw(X, torch.zeros(4, 9))
    with pytest.raises(TypeError, match="assign"):
        ops.kmeans_update_raw(X, a.long(), C)
    with pytest.raises(TypeError, match="assign"):
        ops.kmeans_update_raw(X, a[:9], C)
    with pytest.raises(TypeError, match="counts"):
        ops.kmeans_update_raw(X, a, C, counts=torch.zeros(4))
    with pytest.raises(TypeError, match="dist2"):
        ops.kmeans_assign_raw(X, C, dist2=torch.zeros(9))
    with pytest.raises(TypeError, match="inertia"):
        ops.kmeans_raw(X, C, 3, inertia=torch.zeros(3))
    with pytest.raises(ValueError, match="niter = -1"):
        ops.kmeans_raw(X, C, -1)
    with pytest.raises(ValueError, match="width 300"):
        ops.kmeans_assign_raw(torch.zeros(10, 300), torch.zeros(4, 300))
    with pytest.raises(ValueError, match="must be \\[N, d\\]"):
        ops.kmeans_assign_raw(torch.zeros(10), C)
    with pytest.raises(TypeError, match="contiguous rows"):
        ops.kmeans_assign_raw(torch.zeros(8, 10).t(), C)
    with pytest.raises(ValueError, match="not built"):
        ops.kmeans_workspace(10, 4, 257, "cpu")
