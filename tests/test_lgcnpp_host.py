"""LightGCN++, host side: the fixture regenerates from the reference, the adjacency builder reproduces the reference's
D^-alpha A D^-beta bit for bit and shares its cache file, the settings file carries the reference's keys, the plugin resolves
and refuses what it cannot run, header / binding / library agree on the two row-normalisation entry points, the argument
checks of the library and of the wrappers that need no device, and the float64 closed form of the normalisation's backward
(tests/lgcnpp_ref64.py, the yardstick of tests/test_gpu_lgcnpp.py) against float64 autograd."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import lgcnpp_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lgcnpp_small.npz")
# where the reference tree lives is stated once, by the golden generators (oracle/gen_golden.py)
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
REF_KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[10, 20]", training_epochs="1000", interval="1",
                early_stopping="10", embedding_size="64", batch_size="2048", test_batch_size="2048", learn_rate="0.001",
                reg_lambda="0.0001", GCN_layer="3", gamma="0.2", alpha="0.6", beta="-0.1", sparsity_test="0")
SETTINGS = {"def": (0.6, -0.1, 0.2), "skew": (0.2, 0.9, 0.5)}  # tag -> (alpha, beta, gamma)


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN_pp.txt"), "LightGCN_pp")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _small_data(tmp_path, g, cfg):
    import utility.utility_data.data_loader as data_loader

    d = tmp_path / "small"
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    return data_loader.Data(str(d), cfg)


def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_lgcnpp.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    a, b = np.load(FIXTURE, allow_pickle=False), np.load(str(tmp_path / "lgcnpp_small.npz"), allow_pickle=False)
    assert sorted(a.keys()) == sorted(b.keys())
    for k in a.keys():  # every array byte for byte (the container's compressed stream is not compared)
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_fixture_holds_both_settings():
    g = np.load(FIXTURE)
    for tag, abg in SETTINGS.items():
        assert tuple(g[tag + "_abg"]) == abg
        assert g[tag + "_loss"].shape == (2,) and g[tag + "_traj_loss"].shape == (3, 2)
        assert g[tag + "_grad_user"].shape == g[tag + "_traj_user"].shape == (300, 64)
        assert g[tag + "_grad_item"].shape == g[tag + "_traj_item"].shape == (250, 64)
        assert g[tag + "_rating"].shape == (32, 250)
        assert np.isfinite(g[tag + "_loss"]).all() and np.isfinite(g[tag + "_traj_user"]).all()
        # every user and all items but the four without a training edge receive gradient
        assert (np.abs(g[tag + "_grad_user"]).sum(axis=1) > 0).sum() == 300
        assert (np.abs(g[tag + "_grad_item"]).sum(axis=1) > 0).sum() == 246
        assert g[tag + "_adj_data"].dtype == np.float32 and g[tag + "_adj_indptr"].shape == (551,)
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96


@pytest.mark.parametrize("tag", sorted(SETTINGS))
def test_builder_reproduces_the_reference_adjacency_bit_for_bit(tag, tmp_path, golden_small, capsys):
    import scipy.sparse as sp

    import utility.utility_data.data_graph as data_graph

    g = np.load(FIXTURE)
    alpha, beta, _ = SETTINGS[tag]
    data = _small_data(tmp_path, golden_small, _cfg())
    mat = data_graph.sparse_adjacency_matrix_asymmetric(data, alpha, beta)
    assert "constructed" in capsys.readouterr().out
    assert sp.isspmatrix_csr(mat) and mat.dtype == np.float32 and mat.shape == (550, 550)
    assert np.array_equal(mat.indptr, g[tag + "_adj_indptr"]) and np.array_equal(mat.indices, g[tag + "_adj_indices"])
    assert np.array_equal(mat.data.view(np.uint32), g[tag + "_adj_data"].view(np.uint32))
    # the four items without a training edge: empty rows (and, the structure being symmetric, empty columns)
    empty = np.flatnonzero(np.diff(mat.indptr) == 0)
    assert len(empty) == 4 and (empty >= 300).all() and not np.isin(mat.indices, empty).any()
    assert np.isfinite(mat.data).all() and (mat.data > 0).all()
    # alpha != beta: not its own transpose
    assert abs(mat - mat.T).max() > 0.1
    # the cache file carries the reference's name and is what the second call loads
    name = "pre_A_%s_%s.npz" % (alpha, beta)
    assert name in ("pre_A_0.6_-0.1.npz", "pre_A_0.2_0.9.npz") and (tmp_path / "small" / name).exists()
    again = data_graph.sparse_adjacency_matrix_asymmetric(data, alpha, beta)
    assert "loading completed" in capsys.readouterr().out
    assert np.array_equal(again.indptr, mat.indptr) and np.array_equal(again.indices, mat.indices)
    assert np.array_equal(again.data.view(np.uint32), mat.data.view(np.uint32))
    # the other builders' files are untouched names
    assert not (tmp_path / "small" / "pre_A.npz").exists()


def test_settings_file_carries_the_reference_keys():
    import utility.utility_function.tools as tools

    cfg = _cfg()
    assert dict(cfg) == REF_KEYS
    if os.path.isdir(os.path.join(REF, "configure")):
        assert dict(tools.read_configuration(os.path.join(REF, "configure", "LightGCN_pp.txt"), "LightGCN_pp")) == REF_KEYS


def test_plugin_resolves_and_refuses_what_it_cannot_run(tmp_path):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader

    mod = importlib.import_module("models.LightGCN_pp")
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.LightGCN_pp
    assert cls.supports_fused_step and cls.n_fused_losses == 2
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_train_step", "fused_loss_and_grad",
                 "_eval_panels"):
        assert callable(getattr(cls, name))
    from idgrec_amd.modeling import PackedRecommender

    assert issubclass(cls, PackedRecommender) and cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="LightGCN_pp needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))
    assert "LightGCN_pp" in open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0]


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1)) == 142
    for name, n_args in (("idg_rows_normalize_f32", 7), ("idg_rows_normalize_bwd_f32", 11)):
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert len(proto.group(1).split(",")) == n_args == len(native.PROTOTYPES[name][1])
        assert hasattr(native.lib, name)
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_rownorm.hip"' in build.split("SOURCES")[1].split("]")[0]


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    X0, Y0, N0, G0, A0, O0 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000  # 10 x 64 floats = 2560 bytes each

    def fwd(X=X0, n=10, d=64, eps=1e-12, Y=Y0, norms=N0):
        return L.idg_rows_normalize_f32(X, n, d, eps, Y, norms, None)

    def bwd(T=X0, Y=Y0, norms=N0, eps=1e-12, G=G0, a=0.2, add2=A0, out=O0, n=10, d=64):
        return L.idg_rows_normalize_bwd_f32(T, Y, norms, eps, G, a, add2, out, n, d, None)

    sizes = ((dict(n=0), "bad sizes"), (dict(n=-4), "bad sizes"), (dict(n=1 << 31), "bad sizes"), (dict(d=0), "d = 0"),
             (dict(d=513), "d = 513"), (dict(d=-8), "d = -8"), (dict(eps=0.0), "eps"), (dict(eps=-1e-12), "eps"),
             (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"))
    cases = {
        fwd: ((dict(X=None), "NULL"), (dict(Y=None), "NULL"), (dict(norms=None), "NULL"), (dict(X=X0 + 4), "misaligned"),
              (dict(Y=Y0 + 8), "misaligned"), (dict(norms=N0 + 2), "misaligned"),
              (dict(Y=X0 + 16), "overlaps X"), (dict(Y=X0 + 2544), "overlaps X"), (dict(Y=X0 - 2544), "overlaps X"),
              (dict(norms=X0), "norms overlaps"), (dict(norms=X0 + 2556), "norms overlaps"), (dict(norms=Y0 + 256), "norms overlaps"),
              (dict(X=N0, Y=N0), "norms overlaps")),
        bwd: ((dict(T=None), "NULL"), (dict(Y=None), "NULL"), (dict(norms=None), "NULL"), (dict(out=None), "NULL"),
              (dict(T=X0 + 4), "misaligned"), (dict(Y=Y0 + 8), "misaligned"), (dict(G=G0 + 4), "misaligned"),
              (dict(add2=A0 + 12), "misaligned"), (dict(out=O0 + 8), "misaligned"), (dict(norms=N0 + 1), "misaligned"),
              (dict(out=Y0), "out overlaps Y or norms"), (dict(out=Y0 + 16), "out overlaps Y or norms"),
              (dict(out=N0), "out overlaps Y or norms"), (dict(out=N0 - 2544), "out overlaps Y or norms"),
              (dict(out=X0 + 16), "without being it"), (dict(out=G0 + 32), "without being it"),
              (dict(out=A0 - 16), "without being it"), (dict(out=Y0, G=None, add2=None), "out overlaps Y or norms")),
    }
    for fn, who in ((fwd, "idg_rows_normalize_f32"), (bwd, "idg_rows_normalize_bwd_f32")):
        for kw, word in cases[fn] + sizes:
            assert fn(**kw) == -1, (who, kw)
            msg = L.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    X = torch.zeros(10, 8)
    n = torch.zeros(10)
    for call in (lambda: ops.rows_normalize_raw(X), lambda: ops.rows_normalize_bwd_raw(X, X, n), lambda: ops.rows_normalize(X),
                 lambda: ops.propagate_normalized(None, X, 2, 0.2)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    with pytest.raises(TypeError, match="float32"):
        ops.rows_normalize_raw(X.double())
    with pytest.raises(TypeError, match="float32"):
        ops.rows_normalize(X.double())
    with pytest.raises(TypeError, match="float32"):
        ops.propagate_normalized(None, X.half(), 2, 0.2)
    with pytest.raises(TypeError, match="contiguous float32"):
        ops.rows_normalize_raw(torch.zeros(8, 10).t())
    with pytest.raises(ValueError, match=r"must be \[n, d\]"):
        ops.rows_normalize_raw(torch.zeros(10))
    with pytest.raises(ValueError, match="width 513"):
        ops.rows_normalize_raw(torch.zeros(2, 513))
    with pytest.raises(ValueError, match="0 rows"):
        ops.rows_normalize_raw(torch.zeros(0, 8))
    with pytest.raises(TypeError, match="Y must be"):
        ops.rows_normalize_raw(X, Y=torch.zeros(10, 9))
    with pytest.raises(TypeError, match="norms must be"):
        ops.rows_normalize_raw(X, norms=torch.zeros(9))
    with pytest.raises(TypeError, match="norms must be"):
        ops.rows_normalize_bwd_raw(X, X, n.double())
    with pytest.raises(TypeError, match="Y and norms"):
        ops.rows_normalize_bwd_raw(X, None, n)
    with pytest.raises(TypeError, match="G must be"):
        ops.rows_normalize_bwd_raw(X, X, n, G=X.double())
    with pytest.raises(TypeError, match="add2 must be"):
        ops.rows_normalize_bwd_raw(X, X, n, add2=torch.zeros(10, 4))
    with pytest.raises(TypeError, match="out must be"):
        ops.rows_normalize_bwd_raw(X, X, n, out=torch.zeros(8, 10).t())
    for K in (0, -2):
        with pytest.raises(ValueError, match="K = %d layers" % K):
            ops.propagate_normalized(None, X, K, 0.2)


@pytest.mark.parametrize("d", [7, 64])
def test_closed_form_of_the_backward_equals_float64_autograd(d):
    gen = torch.Generator().manual_seed(d)
    X = torch.randn(50, d, dtype=torch.float64, generator=gen) * 0.3
    T = torch.randn(50, d, dtype=torch.float64, generator=gen)
    x = X.clone().requires_grad_(True)
    y = x / (torch.norm(x, dim=1) + ref.EPS)[:, None]
    (y * T).sum().backward()
    Y, n = ref.rownorm64(X)
    assert torch.equal(Y, y.detach())
    J = ref.rownorm_bwd64(T, Y, n)
    err = (J - x.grad).abs().max() / x.grad.abs().max()
    print("closed form vs autograd: %.3g of the largest entry" % float(err))
    assert float(err) <= 1e-12
    # the other terms are plain sums
    G, A2 = torch.randn(50, d, dtype=torch.float64, generator=gen), torch.randn(50, d, dtype=torch.float64, generator=gen)
    assert torch.equal(ref.rownorm_bwd64(T, Y, n, G=G, a=0.2, add2=A2), J + 0.2 * G + A2)
    assert bool((ref.rownorm_bwd_abs64(T, Y, n, G=G, a=-0.2, add2=A2) >= ref.rownorm_bwd64(T, Y, n, G=G, a=-0.2, add2=A2).abs()).all())


def test_closed_form_of_the_backward_at_a_zero_row():
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(6, 16, dtype=torch.float64, generator=gen)
    X[0] = 0
    X[4] = 0
    T = torch.randn(6, 16, dtype=torch.float64, generator=gen)
    x = X.clone().requires_grad_(True)
    y = x / (torch.norm(x, dim=1) + ref.EPS)[:, None]
    (y * T).sum().backward()
    Y, n = ref.rownorm64(X)
    assert float(n[0]) == 0.0 and bool((Y[0] == 0).all()) and bool((Y[4] == 0).all())
    J = ref.rownorm_bwd64(T, Y, n)
    assert torch.equal(J[0], T[0] / ref.EPS) and torch.equal(J[4], T[4] / ref.EPS)
    # torch's norm has gradient 0 at the origin: autograd says t / e there as well
    assert torch.equal(x.grad[0], T[0] / ref.EPS) and torch.equal(x.grad[4], T[4] / ref.EPS)
    rows = [1, 2, 3, 5]
    assert float((J[rows] - x.grad[rows]).abs().max()) <= 1e-12 * float(x.grad[rows].abs().max())
    assert torch.equal(ref.rownorm_bwd_abs64(T, Y, n)[0], T[0].abs() / ref.EPS)
