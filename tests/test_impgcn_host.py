"""IMP-GCN, host side: the fixture regenerates from the reference and holds both settings; tests/impgcn_ref64.py — the float64
statement tests/test_gpu_impgcn.py holds the kernels against — reproduces the reference's membership, evaluation panels,
rating, losses, gradients and three-step Adam trajectory, and `small` has no near-tied row, so those comparisons are
unconditional; the settings file carries the reference's keys; the plugin resolves through main.py's import path and does not
offer its fused step off the device, for d = 128 or for group = 9; header / binding / library agree on the entry points of
csrc/idg_group.hip; every argument check of theirs comes before any device work; the wrappers' errors."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import impgcn_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "impgcn_small.npz")
# where the reference tree lives is stated once, by the golden generators (oracle/gen_golden.py)
REF = os.environ.get("IDG_REFERENCE") or re.search(r'"IDG_REFERENCE", "([^"]+)"',
                                                   open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()).group(1)
REF_KEYS = dict(dataset_path="./dataset/", dataset="yelp2018", top_K="[20, 40]", training_epochs="1000", early_stopping="10",
                interval="10", embedding_size="64", batch_size="2048", test_batch_size="200", learn_rate="0.001",
                reg_lambda="0.0001", GCN_layer="6", group="3", sparsity_test="0")
SETTINGS = {"def": (3, 6), "two": (2, 3)}  # tag -> (group, GCN_layer)
RTOL = 1e-4  # tests/test_gcmc_host.py
REG, LR = 1e-4, 1e-3  # configure/IMPGCN.txt, what the goldens were taken with
U, I, N = 300, 250, 550


def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "IMPGCN.txt"), "IMPGCN")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_regenerates_from_the_reference(tmp_path):
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("needs the reference tree (%s)" % REF)
    env = dict(os.environ, IDG_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "scripts", "gen_golden_impgcn.py")], check=True, env=env,
                   cwd=ROOT, stdout=subprocess.DEVNULL)
    a, b = np.load(FIXTURE, allow_pickle=False), np.load(str(tmp_path / "impgcn_small.npz"), allow_pickle=False)
    assert sorted(a.keys()) == sorted(b.keys())
    for k in a.keys():  # every array byte for byte (the container's compressed stream is not compared)
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_fixture_holds_both_settings():
    g = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert g["init_user"].shape == (U, 64) and g["init_item"].shape == (I, 64)
    assert g["fc_weight"].shape == (64, 64) and g["fc_bias"].shape == (64,)
    for tag, (G, L) in SETTINGS.items():
        assert g[tag + "_fc_group_weight"].shape == (G, 64) and g[tag + "_fc_group_bias"].shape == (G,)
        full = (1 << G) - 1
        for key in ("_eval_member", "_member"):
            m = g[tag + key]
            assert m.shape == (N,) and m.dtype == np.uint8 and (m[U:] == full).all() and (m[:U] >= 1).all() and (m[:U] <= full).all()
        assert g[tag + "_traj_member"].shape == (3, N)
        # dropout off: one group per user (no exact tie among `small`'s scores); on: ties are common
        assert (np.bincount(g[tag + "_eval_member"][:U], minlength=full + 1)[[1 << k for k in range(G)]].sum()) == U
        multi = np.mean([bin(int(x)).count("1") > 1 for x in g[tag + "_member"][:U]])
        print("%s: share of multi-group users under the masks %.3f" % (tag, multi))
        assert 0 < multi < 1  # (which rows: test_float64_statement_reproduces_the_references_step)
        assert g[tag + "_loss"].shape == (2,) and g[tag + "_traj_loss"].shape == (3, 2)
        assert g[tag + "_grad_user"].shape == g[tag + "_traj_user"].shape == g[tag + "_eval_user"].shape == (U, 64)
        assert g[tag + "_grad_item"].shape == g[tag + "_traj_item"].shape == g[tag + "_eval_item"].shape == (I, 64)
        assert g[tag + "_rating"].shape == (32, I)
        # no gradient reaches fc / fc_group in the reference, and Adam leaves them where they were
        assert g[tag + "_fc_grad_is_none"].tolist() == [True] * 4 and g[tag + "_traj_fc_unchanged"].tolist() == [True] * 4
    b = g["batch"]
    assert b.shape == (96, 3) and len(set(b[:, 0].tolist())) < 96 and len(set(b[:, 1].tolist())) < 96
    assert g["traj_batches"].shape == (768, 3) and g["rating_users"].shape == (32,)
    assert len(set(g["grad_streams"].tolist()) | set(g["traj_streams"].reshape(-1).tolist())) == 8


# ------------------------------------------------------------------------------- the float64 statement is the reference's
def _setting(golden_small, tag):
    g, gs = np.load(FIXTURE), golden_small
    assert int(gs["num_users"]) == U and int(gs["num_items"]) == I
    A = ref.dense_operator(gs["adj_indptr"], gs["adj_indices"], gs["adj_data"], (N, N))
    E0 = torch.from_numpy(np.concatenate([g["init_user"], g["init_item"]]))
    small = tuple(torch.from_numpy(g[k]) for k in ("fc_weight", "fc_bias", tag + "_fc_group_weight", tag + "_fc_group_bias"))
    return g, A, E0, small


def _masks(g, streams, G):
    seed = int(g["mask_seed"])
    return ref.keep_mask(ref.P_DROP, seed, int(streams[0]), N, 64), ref.keep_mask(ref.P_DROP, seed, int(streams[1]), N, G)


@pytest.mark.parametrize("tag", sorted(SETTINGS))
def test_float64_statement_reproduces_the_references_evaluation(tag, golden_small):
    g, A, E0, small = _setting(golden_small, tag)
    G, L = SETTINGS[tag]
    for dtype in (torch.float64, torch.float32):
        scores, member, near = ref.assign64(E0, A.to(dtype) @ E0.to(dtype), *small, U, dtype=dtype)
        assert scores.dtype == dtype and member.dtype == torch.uint8
        assert int(near.sum()) == 0  # `small` has NO near-tied row: everything below is unconditional
        assert np.array_equal(member.numpy(), g[tag + "_eval_member"])
    final = ref.final64(A, E0, member, G, L)
    np.testing.assert_allclose(final[:U].numpy(), g[tag + "_eval_user"], rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(final[U:].numpy(), g[tag + "_eval_item"], rtol=RTOL, atol=1e-7)
    users = torch.from_numpy(g["rating_users"])
    np.testing.assert_allclose(torch.sigmoid(final[users] @ final[U:].t()).numpy(), g[tag + "_rating"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("tag", sorted(SETTINGS))
def test_float64_statement_reproduces_the_references_step(tag, golden_small):
    g, A, E0, small = _setting(golden_small, tag)
    G, L = SETTINGS[tag]
    m1, m2 = _masks(g, g["grad_streams"], G)
    scores, member, near = ref.assign64(E0, A @ E0.double(), *small, U, m1, m2)
    assert int(near.sum()) == 0 and np.array_equal(member.numpy(), g[tag + "_member"])
    # ties by value: a row whose scores were all dropped belongs to every group
    dropped = (m2[:U] == 0).all(dim=1)
    assert int(dropped.sum()) > 0 and (member[:U][dropped] == (1 << G) - 1).all()
    b = torch.from_numpy(g["batch"])
    member = torch.from_numpy(g[tag + "_member"])
    losses, gE0, final, gf = ref.step64(A, E0, member, b[:, 0], b[:, 1], b[:, 2], G, L, REG, U)
    assert losses.dtype == gE0.dtype == final.dtype == torch.float64 and final.shape == (N, 64)
    np.testing.assert_allclose(losses.numpy(), g[tag + "_loss"], rtol=RTOL)
    np.testing.assert_allclose(gE0[:U].numpy(), g[tag + "_grad_user"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(gE0[U:].numpy(), g[tag + "_grad_item"], rtol=1e-3, atol=1e-8)
    # the issue's closed form: d E0 = (G / L) gF + (1 / L) sum_g sum_l A_g^l gF + the regulariser's rows, in Horner form
    H = None
    for _ in range(L - 1):
        if H is None:
            H = ref.propagate64(A, gf, member, G, 1)[0]
        else:
            H = [ref.propagate64(A, H[k], member, G, 1, V=gf)[0][k] for k in range(G)]
    horner = (G / L) * gf + (sum(H) / L if H is not None else 0)
    _, _, ge = ref.bpr64(final, E0, U, b[:, 0], b[:, 1], b[:, 2], REG, reg_users=True)
    assert float((horner + ge - gE0).abs().max()) < 1e-12 * float(gE0.abs().max()) + 1e-18
    # the same expressions in float32: the yardstick the GPU file measures the kernels with
    l32, g32, f32, _ = ref.step64(A, E0, member, b[:, 0], b[:, 1], b[:, 2], G, L, REG, U, dtype=torch.float32)
    assert l32.dtype == g32.dtype == f32.dtype == torch.float32
    e_ref, e_f32 = ref.errors(np.concatenate([g[tag + "_grad_user"], g[tag + "_grad_item"]]), gE0, g32)
    print("%s d E0: the reference %.2e, the float32 composition %.2e of max from float64" % (tag, e_ref, e_f32))
    assert e_f32 < 1e-5


@pytest.mark.parametrize("tag", sorted(SETTINGS))
def test_float64_statement_reproduces_the_references_trajectory(tag, golden_small):
    """Three step64 + adam64 steps on the fixture's three 256-row batches, each fed the reference's membership of that step
    (which assign64 reproduces from the current table: no near-tied row).  Losses at RTOL.  The table: the trajectory criterion
    of tests/test_gccf_host.py — fewer than one element in a thousand outside rtol 1e-4 / atol 1e-6, none further than a
    third of the total movement (three Adam steps move an element by at most 3 lr)."""
    g, A, E0, small = _setting(golden_small, tag)
    G, L = SETTINGS[tag]
    tri = torch.from_numpy(g["traj_batches"])
    cur, grads, losses = E0.double(), [], []
    for i in range(3):
        b = tri[i * 256:(i + 1) * 256]
        m1, m2 = _masks(g, g["traj_streams"][i], G)
        _, member, near = ref.assign64(cur, A @ cur, *small, U, m1, m2)
        assert int(near.sum()) == 0 and np.array_equal(member.numpy(), g[tag + "_traj_member"][i]), i
        ll, gE0, _, _ = ref.step64(A, cur, member, b[:, 0], b[:, 1], b[:, 2], G, L, REG, U)
        losses.append(ll.numpy())
        grads.append(gE0)
        cur = ref.adam64(E0, grads, lr=LR)[-1][0]
    np.testing.assert_allclose(np.array(losses), g[tag + "_traj_loss"], rtol=RTOL)
    want = np.concatenate([g[tag + "_traj_user"], g[tag + "_traj_item"]])
    mine = cur.numpy()
    moved = np.abs(want - E0.numpy()).max()
    off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
    print("%s: moved %.3g, off %.3g, max %.3g" % (tag, moved, off.mean(), np.abs(mine - want).max()))
    assert 1e-4 < moved <= 3.01 * LR
    assert off.mean() < 1e-3 and np.abs(mine - want).max() < LR


def test_membership_conventions():
    """Ties by VALUE: -0.0 against +0.0, two equal positive scores, every score dropped; items belong to every group."""
    s = torch.tensor([[-0.0, 0.0, -1.0], [2.5, 1.0, 2.5], [0.0, 0.0, 0.0], [-3.0, -2.0, -1.0], [9.0, 9.0, 9.0]], dtype=torch.float64)
    assert ref.argmax_set(s, 4).tolist() == [0b011, 0b101, 0b111, 0b100, 0b111]
    assert ref.groups_of(torch.tensor([5, 0, 7], dtype=torch.uint8), 3).tolist() == [[True, False, True], [False] * 3, [True] * 3]
    assert ref.bits_of(ref.groups_of(torch.arange(8, dtype=torch.uint8), 3)).tolist() == list(range(8))


# ------------------------------------------------------------------------------------------ settings, plugin, main.py
def test_settings_file_carries_the_reference_keys():
    import utility.utility_function.tools as tools

    cfg = _cfg()
    assert dict(cfg) == REF_KEYS and list(dict(cfg)) == list(REF_KEYS)
    if os.path.isdir(os.path.join(REF, "configure")):
        assert dict(tools.read_configuration(os.path.join(REF, "configure", "IMPGCN.txt"), "IMPGCN")) == REF_KEYS


def test_plugin_resolves_and_does_not_fuse_off_the_device(tmp_path, monkeypatch):
    import idgrec_amd.synth as S
    import utility.utility_data.data_loader as data_loader
    from idgrec_amd.modeling import EngineStep, PackedRecommender

    mod = importlib.import_module("models.IMPGCN")  # main.py: importlib.import_module('models.' + model_name).Trainer
    assert callable(mod.Trainer) and callable(mod.Trainer.train)
    cls = mod.IMPGCN
    assert cls.supports_fused_step and cls.n_fused_losses == 2
    for name in ("aggregate", "forward", "get_rating_for_test", "topk_for_test", "fused_step_available", "fused_train_step",
                 "fused_loss_and_grad", "prefetch_batch", "_eval_panels", "membership"):
        assert callable(getattr(cls, name)), name
    assert issubclass(cls, PackedRecommender) and issubclass(cls, EngineStep)
    assert cls._eval_panels is not PackedRecommender._eval_panels
    S.make_dataset(str(tmp_path), "tiny", n_test=1)
    cfg = _cfg(dataset="tiny", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(tmp_path / "tiny"), cfg)
    with pytest.raises(RuntimeError, match="IMPGCN needs an MI355X"):
        cls(cfg, data, torch.device("cpu"))
    for layers in ("0", "-1"):
        with pytest.raises(ValueError, match="GCN_layer >= 1"):
            cls(dict(cfg, GCN_layer=layers), data, torch.device("cpu"))
    with pytest.raises(ValueError, match="group >= 1"):
        cls(dict(cfg, group="0"), data, torch.device("cpu"))
    # off the device the graph cannot be attached; with that step left out the model stands, on the CPU, and must not offer
    # its fused step
    monkeypatch.setattr(PackedRecommender, "attach_graph", lambda self, sp_mat: None)
    torch.manual_seed(0)
    m = cls(cfg, data, torch.device("cpu"))
    names = [k for k, _ in m.named_parameters()]
    assert names == ["user_embedding.weight", "item_embedding.weight", "fc.weight", "fc.bias", "fc_group.weight", "fc_group.bias"]
    assert [p is q for p, q in zip(m.parameters(), m._engine_params())] == [True] * 6
    assert tuple(m.fc_group.weight.shape) == (3, 64) and not m._storage.is_cuda and m.fused_step_available() is False
    wide = cls(dict(cfg, embedding_size="128"), data, torch.device("cpu"))
    nine = cls(dict(cfg, group="9"), data, torch.device("cpu"))
    assert wide.fused_step_available() is False and nine.fused_step_available() is False
    # the same judgement with the storage claimed to be on the device: the width and the group count alone rule it out
    def on_device(model, d):
        class OnDevice:
            is_cuda, shape = True, (model._storage.shape[0], d)
        monkeypatch.setattr(model, "_storage", OnDevice)

    on_device(m, 64), on_device(wide, 128), on_device(nine, 64)
    assert m.fused_step_available() is True and wide.fused_step_available() is False and nine.fused_step_available() is False
    eight = cls(dict(cfg, group="8", GCN_layer="1"), data, torch.device("cpu"))
    on_device(eight, 64)
    assert eight.fused_step_available() is True


def test_main_names_impgcn_as_implemented():
    assert "IMPGCN" in re.split(r"[,.\s]+", open(os.path.join(ROOT, "main.py")).read().split("Implemented:")[1].split("\n")[0])


# ------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = (("idg_group_assign_f32", 18), ("idg_grouped_spmm_chunk", 1), ("idg_grouped_spmm_workspace_bytes", 2),
                ("idg_grouped_spmm_f32", 23), ("idg_group_grad_f32", 10))


def test_header_binding_and_library_agree_on_the_entry_points():
    from idgrec_amd import native

    hdr = open(os.path.join(ROOT, "include", "idgrec.h")).read()
    assert native.lib.idg_version() == native.ABI_VERSION == int(re.search(r"#define IDG_VERSION (\d+)", hdr).group(1))
    for name, n_args in ENTRY_POINTS:
        proto = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert proto, name
        n_bound = len(native.PROTOTYPES[name][1])
        assert len(proto.group(1).split(",")) == n_args and n_bound == (0 if proto.group(1).strip() == "void" else n_args), name
        assert hasattr(native.lib, name)
    build = open(os.path.join(ROOT, "id-grec_amd", "build.py")).read()
    assert '"idg_group.hip"' in build.split("SOURCES")[1].split("]")[0]
    chunk = int(re.search(r"#define IDG_GROUP_CHUNK (\d+)", hdr).group(1))
    assert native.lib.idg_grouped_spmm_chunk() == chunk == 512
    assert native.lib.idg_grouped_spmm_workspace_bytes(7, 3) == 7 * 3 * 64 * 4
    for bad in ((0, 3), (-1, 3), (7, 0), (7, 9)):
        assert native.lib.idg_grouped_spmm_workspace_bytes(*bad) == 0


def test_library_argument_checks_come_before_any_device_work():
    """IDG_E_INVALID with a message for everything the entry points can judge on the host.  Every call here is refused: the
    pointers are made-up addresses that no kernel may ever see."""
    from idgrec_amd import native

    L = native.lib
    nan = float("nan")
    # n = 10: a panel is 2560 bytes, W_fc 16384, a bias 256, W_grp 768, member 10, scores 120
    EGO, SIDE, WFC, BFC, WGRP, BGRP, MEM, SC = 0x10000, 0x20000, 0x30000, 0x38000, 0x39000, 0x3A000, 0x40000, 0x50000

    def assign(ego=EGO, side=SIDE, Wfc=WFC, bfc=BFC, Wgrp=WGRP, bgrp=BGRP, n=10, d=64, G=3, nu=5, p=0.4, member=MEM, scores=SC):
        return L.idg_group_assign_f32(ego, side, Wfc, bfc, Wgrp, bgrp, n, d, G, nu, 0.01, p, 1234, 1, 2, member, scores, None)

    # a [3, 10, 64] grouped panel is 7680 bytes; indptr 88, indices / values 4 nnz; a bitmap 4; the workspace 2 * 3 * 256
    PTR, IDX, VAL, X, V, Y, SIN, S = 0x100000, 0x110000, 0x120000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    XR, VR, LR_, LC, WS = 0x700000, 0x710000, 0x720000, 0x730000, 0x800000

    def spmm(n=10, nnz=40, indptr=PTR, indices=IDX, values=VAL, d=64, G=3, member=MEM, X=X, xgs=0, x_rows=None, V=None, v_rows=None,
             Y=Y, ygs=640, S_in=None, S=S, long_rows=None, chunk0=None, n_long=0, n_chunks=0, ws=None):
        return L.idg_grouped_spmm_f32(n, nnz, indptr, indices, values, d, G, member, X, xgs, x_rows, V, v_rows, Y, ygs, S_in, S,
                                      long_rows, chunk0, n_long, n_chunks, ws, None)

    def grad(S=S, gF=X, GE=V, rows=XR, n=10, d=64, out=Y):
        return L.idg_group_grad_f32(S, 0.5, gF, 0.5, GE, rows, n, d, out, None)

    sizes = ((dict(n=0), "bad sizes"), (dict(n=-4), "bad sizes"), (dict(n=1 << 31), "bad sizes"), (dict(d=0), "d = 64 only (got 0)"),
             (dict(d=32), "d = 64 only (got 32)"), (dict(d=128), "d = 64 only (got 128)"), (dict(d=-64), "d = 64 only"))
    groups = ((dict(G=0), "outside 1 .. 8"), (dict(G=9), "outside 1 .. 8"), (dict(G=-3), "outside 1 .. 8"))
    cases = {
        assign: ((dict(ego=None), "NULL"), (dict(side=None), "NULL"), (dict(Wfc=None), "NULL"), (dict(bfc=None), "NULL"),
                 (dict(Wgrp=None), "NULL"), (dict(bgrp=None), "NULL"), (dict(member=None), "NULL"),
                 (dict(ego=EGO + 4), "misaligned"), (dict(side=SIDE + 8), "misaligned"), (dict(Wfc=WFC + 4), "misaligned"),
                 (dict(bfc=BFC + 2), "misaligned"), (dict(Wgrp=WGRP + 1), "misaligned"), (dict(bgrp=BGRP + 3), "misaligned"),
                 (dict(scores=SC + 2), "misaligned"),
                 (dict(nu=-1), "num_users"), (dict(nu=11), "num_users"),
                 (dict(p=-0.1), "drop probability"), (dict(p=1.0), "drop probability"), (dict(p=nan), "drop probability"),
                 (dict(member=EGO), "overlaps"), (dict(member=EGO + 2559), "overlaps"), (dict(member=SIDE - 9), "overlaps"),
                 (dict(member=WFC + 16383), "overlaps"), (dict(member=BFC + 255), "overlaps"), (dict(member=WGRP + 767), "overlaps"),
                 (dict(member=BGRP + 11), "overlaps"), (dict(scores=EGO + 2556), "overlaps"), (dict(scores=SIDE - 116), "overlaps"),
                 (dict(scores=WGRP), "overlaps"), (dict(scores=BGRP - 116), "overlaps"),
                 (dict(scores=MEM - 116), "overlap"), (dict(scores=MEM + 8), "overlap")) + sizes + groups,
        spmm: ((dict(indptr=None), "NULL"), (dict(member=None), "NULL"), (dict(X=None), "NULL"), (dict(Y=None, S=None), "NULL"),
               (dict(indices=None), "NULL"), (dict(values=None), "NULL"),
               (dict(nnz=-1), "bad sizes"),
               (dict(xgs=636), "x_group_stride"), (dict(xgs=-640), "x_group_stride"), (dict(xgs=642), "multiples of 4"),
               (dict(ygs=636), "y_group_stride"), (dict(ygs=0), "y_group_stride"), (dict(ygs=642), "multiples of 4"),
               (dict(xgs=640, x_rows=XR), "SHARED X only"), (dict(v_rows=VR), "v_rows without V"), (dict(S=None, S_in=SIN), "S_in without S"),
               (dict(X=X + 4), "misaligned"), (dict(V=V + 8), "misaligned"), (dict(Y=Y + 4), "misaligned"), (dict(S=S + 12), "misaligned"),
               (dict(S_in=SIN + 4), "misaligned"), (dict(indptr=PTR + 4), "misaligned"), (dict(indices=IDX + 2), "misaligned"),
               (dict(values=VAL + 1), "misaligned"), (dict(x_rows=XR + 2), "misaligned"), (dict(V=V, v_rows=VR + 1), "misaligned"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC, ws=WS + 8), "misaligned"),
               (dict(n_long=1, n_chunks=2), "schedule"), (dict(n_long=1, n_chunks=1, long_rows=LR_, chunk0=LC, ws=WS), "schedule"),
               (dict(n_long=0, n_chunks=2), "schedule"), (dict(n_long=-1), "schedule"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC), "schedule"),
               (dict(Y=X), "overlaps"), (dict(Y=X - 7664), "overlaps"), (dict(Y=X + 2544), "overlaps"), (dict(S=X + 16), "overlaps"),
               (dict(xgs=640, S=X + 7664), "overlaps"),
               (dict(V=V, S=V + 2544), "overlaps"), (dict(S=MEM - 2544), "overlaps"), (dict(Y=PTR + 80), "overlaps"),
               (dict(S=IDX + 144), "overlaps"), (dict(Y=VAL - 7664), "overlaps"), (dict(S_in=SIN, Y=SIN + 16), "overlaps"),
               (dict(x_rows=XR, S=XR - 2544), "overlaps"), (dict(V=V, v_rows=VR, Y=VR), "overlaps"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC, ws=WS, S=LR_), "overlaps"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC, ws=WS, S=LC), "overlaps"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC, ws=X + 2544), "overlaps"),
               (dict(S=Y + 7664), "overlap"), (dict(S=Y - 2544), "overlap"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC, ws=Y + 7664), "overlap"),
               (dict(n_long=1, n_chunks=2, long_rows=LR_, chunk0=LC, ws=S - 1520), "overlap")) + sizes + groups,
        grad: ((dict(gF=None), "NULL"), (dict(GE=None), "NULL"), (dict(rows=None), "NULL"), (dict(out=None), "NULL"),
               (dict(S=S + 4), "misaligned"), (dict(gF=X + 8), "misaligned"), (dict(GE=V + 4), "misaligned"), (dict(out=Y + 4), "misaligned"),
               (dict(rows=XR + 2), "misaligned"),
               (dict(out=X), "overlaps"), (dict(out=V + 2544), "overlaps"), (dict(out=XR - 2544), "overlaps"), (dict(out=S + 16), "overlaps")) + sizes,
    }
    for fn, who in ((assign, "idg_group_assign_f32"), (spmm, "idg_grouped_spmm_f32"), (grad, "idg_group_grad_f32")):
        for kw, word in cases[fn]:
            assert fn(**kw) == -1, (who, kw)
            msg = L.idg_last_error().decode()
            assert who in msg and word in msg, (who, kw, msg)


def test_wrapper_argument_checks():
    from idgrec_amd import ops

    ego, W, b, Wg, bg = torch.zeros(10, 64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(3, 64), torch.zeros(3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.group_assign_raw(ego, ego, W, b, Wg, bg, 5, 0.4, 1, 2, 3)
    for bad in ((ego.double(), ego, W, b, Wg, bg), (ego, ego, W.half(), b, Wg, bg), (ego, ego, W, b, Wg.double(), bg)):
        with pytest.raises(TypeError, match="float32"):
            ops.group_assign_raw(*bad, 5, 0.4, 1, 2, 3)
    for bad in ((torch.zeros(10, 32), torch.zeros(10, 32), W, b, Wg, bg), (ego, torch.zeros(9, 64), W, b, Wg, bg), (torch.zeros(0, 64),) * 2 + (W, b, Wg, bg)):
        with pytest.raises(ValueError, match=r"\[n >= 1, 64\]"):
            ops.group_assign_raw(*bad, 5, 0.4, 1, 2, 3)
    for bad in ((ego, ego, torch.zeros(64, 32), b, Wg, bg), (ego, ego, W, torch.zeros(32), Wg, bg), (ego, ego, W, b, torch.zeros(3, 32), bg),
                (ego, ego, W, b, Wg, torch.zeros(2))):
        with pytest.raises(ValueError, match="do not fit"):
            ops.group_assign_raw(*bad, 5, 0.4, 1, 2, 3)
    with pytest.raises(ValueError, match=r"outside 1 \.\. 8"):
        ops.group_assign_raw(ego, ego, W, b, torch.zeros(9, 64), torch.zeros(9), 5, 0.4, 1, 2, 3)
    for nu in (-1, 11):
        with pytest.raises(ValueError, match="num_users"):
            ops.group_assign_raw(ego, ego, W, b, Wg, bg, nu, 0.4, 1, 2, 3)
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError, match="drop probability"):
            ops.group_assign_raw(ego, ego, W, b, Wg, bg, 5, p, 1, 2, 3)
    with pytest.raises(TypeError, match="uint8"):
        ops.group_assign_raw(ego, ego, W, b, Wg, bg, 5, 0.4, 1, 2, 3, member=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="scores_out"):
        ops.group_assign_raw(ego, ego, W, b, Wg, bg, 5, 0.4, 1, 2, 3, scores_out=torch.zeros(10, 4))
    # the CSR holder judges its host arrays before anything goes to a device
    ptr, idx, val = np.array([0, 1, 2]), np.array([1, 0]), np.ones(2, dtype=np.float32)
    for bad, word in (((np.array([0, 1]), idx, val, 2), "indptr must be"), ((np.array([0, 2, 1]), idx, val, 2), "rise from 0"),
                      ((np.array([1, 1, 2]), idx, val, 2), "rise from 0"), ((ptr, np.array([1, 2]), val, 2), "outside 0 .. 1"),
                      ((ptr, np.array([-1, 0]), val, 2), "outside 0 .. 1"), ((ptr, idx, np.ones(3, dtype=np.float32), 2), "indptr must be")):
        with pytest.raises(ValueError, match=word):
            ops.GroupCsr(*bad, "cpu")
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.GroupCsr(ptr, idx, val, 2, "cpu")
    member = torch.zeros(10, dtype=torch.uint8)
    for call in (lambda: ops.grouped_spmm_raw(None, member, ego, 3, S=ego), lambda: ops.grouped_propagate(None, ego, member, 2, 3)):
        with pytest.raises(TypeError, match="ops.GroupCsr"):
            call()
