"""scripts/gen_golden_na.py — TEST INFRASTRUCTURE.  Goldens for LightCCF and LightCSCF from the imported reference, on the
frozen `small` inputs (300 users, 250 items) with the conventions of oracle/gen_golden.py (whose helpers it imports; nothing
under oracle/ changes).  Runs only where the reference exists, on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_na.py      # -> tests/golden/na_small.npz

Four settings (SETTINGS below): `ccf_mf` — LightCCF, encoder MF, the reference's configure/LightCCF.txt (temperature 0.22,
ssl_lambda 5); `ccf_gcn` — LightCCF, encoder LightGCN, GCN_layer = 2, temperature 0.15 (where the 1e-5 inside the log weighs:
r_i <= exp(-1 / 0.15) = 1.3e-3, and far below it on rows whose user repeats; at 0.1 the reference's own float32 run no longer
meets the trajectory criterion of the tests), reg_lambda 0.01; `cscf_mf` — LightCSCF, encoder MF, configure/LightCSCF.txt's temperature 0.2 and margin 0.7; `cscf_gcn` —
LightCSCF, encoder LightGCN, GCN_layer = 3, margin 0.5, lambda_gamma 2, lambda_reg 0.05 (the list without a BPR entry, the
regulariser large enough to show in the gradient).  The two LightCSCF settings run at embedding_size 32, which keeps the file
under 1 MiB.  The tables are initialised in float32, as the reference does; the model (and its adjacency) is then cast to
float64 and the reference's own forward, backward and torch.optim.Adam run in float64, so the fixture carries no float32
rounding of the reference's; gradients, tables and ratings are stored rounded to float32, the losses as float64.  Stored:
the initial tables per width, a B = 96 batch with forced duplicate users and items, the losses and both .grad,
get_rating_for_test for 32 users, and the losses and tables after three torch.optim.Adam steps on three 256-row batches.
Every LightCSCF forward asserts that no score lies within 1e-5 of the margin.  $IDG_GOLDEN_OUT redirects the output directory.
"""
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import gen_golden as G  # noqa: E402  (puts the reference first on sys.path and imports it)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.LightCCF import LightCCF as RefLightCCF  # noqa: E402
from models.LightCSCF import LightCSCF as RefLightCSCF  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

SETTINGS = {
    "ccf_mf": (RefLightCCF, "LightCCF", dict(encoder="MF", embedding_size=64)),
    "ccf_gcn": (RefLightCCF, "LightCCF", dict(encoder="LightGCN", GCN_layer=2, temperature=0.15, reg_lambda=0.01, embedding_size=64)),
    "cscf_mf": (RefLightCSCF, "LightCSCF", dict(encoder="MF", embedding_size=32)),
    "cscf_gcn": (RefLightCSCF, "LightCSCF", dict(encoder="LightGCN", GCN_layer=3, lambda_margin=0.5, lambda_gamma=2.0, lambda_reg=0.05,
                                                embedding_size=32)),
}
PARAMS = ("user_embedding", "item_embedding")


def hyper(name, cfg):
    """[temperature, GCN_layer, learn_rate, regulariser weight, loss weight, margin (-1: none), embedding_size]."""
    if name == "LightCCF":
        reg, weight, margin = cfg["reg_lambda"], cfg["ssl_lambda"], -1.0
    else:
        reg, weight, margin = cfg["lambda_reg"], cfg["lambda_gamma"], cfg["lambda_margin"]
    return np.array([float(x) for x in (cfg["temperature"], cfg["GCN_layer"], cfg["learn_rate"], reg, weight, margin, cfg["embedding_size"])])


def kink_gap(m, cfg, users, pos):
    """The smallest distance of a score (and of a positive's) from LightCSCF's margin."""
    with torch.no_grad():
        ue, ie = (m.user_embedding.weight, m.item_embedding.weight) if cfg["encoder"] == "MF" else m.aggregate()
        a = torch.nn.functional.normalize(ue[users], dim=1)
        b = torch.nn.functional.normalize(ie[pos], dim=1)
        total = a @ b.T + a @ a.T
        mg = float(cfg["lambda_margin"])
        return float(torch.minimum((total - mg).abs().min(), ((a * b).sum(-1) - mg).abs().min()))


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_na_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        cfg0 = G.base_config("LightCCF", dataset=gname, dataset_path=tmp + "/")
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        bn[9], bn[11] = bp[9], bn[10]  # a negative equal to a positive of the batch, and a repeated negative
        assert int(torch.unique(bu).numel()) < B and int(torch.unique(bp).numel()) < B
        out = {"batch": torch.stack([bu, bp, bn], 1).numpy()}
        tri3 = torch.from_numpy(s1[:3 * 256].copy())
        out["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        out["rating_users"] = test_users.numpy()
        for tag, (cls, name, extra) in SETTINGS.items():
            cfg = G.base_config(name, dataset=gname, dataset_path=tmp + "/", **extra)
            ref_tools.set_seed(G.SEED)
            m = cls(cfg, data, G.CPU)
            assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
            for p in PARAMS:
                key = "init%s_%s" % (cfg["embedding_size"], p)
                init = getattr(m, p).weight.detach().numpy().copy()
                if key in out:
                    assert np.array_equal(out[key], init)
                out[key] = init
            # the float32 initial values, then the reference's own program in float64
            m = m.double()
            m.Graph = m.Graph.double()
            prm = {p: getattr(m, p).weight for p in PARAMS}
            n_losses = 2 if (name == "LightCSCF" and cfg["encoder"] != "MF") else 3
            if name == "LightCSCF":
                assert kink_gap(m, cfg, bu, bp) > 1e-5
            m.zero_grad()
            ll = m(bu, bp, bn)
            assert len(ll) == n_losses
            sum(ll).backward()
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            for p in PARAMS:
                out["%s_grad_%s" % (tag, p)] = prm[p].grad.numpy().astype(np.float32)
            with torch.no_grad():
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy().astype(np.float32)
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj = []
            for i in range(3):
                b = tri3[i * 256:(i + 1) * 256]
                if name == "LightCSCF":
                    assert kink_gap(m, cfg, b[:, 0], b[:, 1]) > 1e-5
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
            out[tag + "_traj_loss"] = np.array(traj)
            for p in PARAMS:
                out["%s_traj_%s" % (tag, p)] = prm[p].detach().numpy().astype(np.float32)
            out[tag + "_hyper"] = hyper(name, cfg)
        G.golden_io.save_npz(os.path.join(G.OUT, "na_small.npz"), **out)
        size = os.path.getsize(os.path.join(G.OUT, "na_small.npz"))
        assert size <= 1 << 20, size
        print("wrote na_small.npz (%d bytes)" % size)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
