"""scripts/gen_golden_sccf.py — TEST INFRASTRUCTURE.  Goldens for SCCF from the imported reference, on the frozen `small`
inputs (300 users, 250 items) with the conventions of oracle/gen_golden.py (whose helpers it imports; nothing under oracle/
changes).  Runs only where the reference exists, on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_sccf.py      # -> tests/golden/sccf_small.npz

Two settings — `mf`: encoder MF, temperature 0.1 (the reference's configure/SCCF.txt); `gcn`: encoder LightGCN, GCN_layer = 2,
temperature 0.2.  The tables are initialised in float32, as the reference does; the model (and its adjacency) is then cast
to float64 and the reference's own forward, backward and torch.optim.Adam run in float64, so the fixture carries no float32
rounding of the reference's; gradients, tables and ratings are stored rounded to float32, the losses as float64.  Stored:
the initial tables (the same in both settings, stored once), a B = 96 batch with forced duplicate users and items and its
two distinct-id counts, the two losses and both .grad, get_rating_for_test for 32 users, and the losses and tables after
three torch.optim.Adam steps on three 256-row batches.  $IDG_GOLDEN_OUT redirects the output directory.
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

from models.SCCF import SCCF as RefSCCF  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

SETTINGS = {
    "mf": dict(encoder="MF", temperature=0.1, GCN_layer=3),
    "gcn": dict(encoder="LightGCN", temperature=0.2, GCN_layer=2),
}
PARAMS = ("user_embedding", "item_embedding")


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_sccf_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        cfg0 = G.base_config("SCCF", dataset=gname, dataset_path=tmp + "/")
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        nu, ni = int(torch.unique(bu).numel()), int(torch.unique(bp).numel())
        assert nu < B and ni < B, (nu, ni)
        out = {"batch": torch.stack([bu, bp, bn], 1).numpy(), "batch_counts": np.array([nu, ni], dtype=np.int64)}
        tri3 = torch.from_numpy(s1[:3 * 256].copy())
        out["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        out["rating_users"] = test_users.numpy()
        for tag, extra in SETTINGS.items():
            cfg = G.base_config("SCCF", dataset=gname, dataset_path=tmp + "/", **extra)
            ref_tools.set_seed(G.SEED)
            m = RefSCCF(cfg, data, G.CPU)
            assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
            for p in PARAMS:
                init = getattr(m, p).weight.detach().numpy().copy()
                if "init_" + p in out:
                    assert np.array_equal(out["init_" + p], init)
                out["init_" + p] = init
            # the float32 initial values, then the reference's own program in float64
            m = m.double()
            m.Graph = m.Graph.double()
            prm = {p: getattr(m, p).weight for p in PARAMS}
            m.zero_grad()
            ll = m(bu, bp, bn)
            assert len(ll) == 2
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
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
            out[tag + "_traj_loss"] = np.array(traj)
            for p in PARAMS:
                out["%s_traj_%s" % (tag, p)] = prm[p].detach().numpy().astype(np.float32)
            out[tag + "_hyper"] = np.array([extra["temperature"], extra["GCN_layer"], float(cfg["learn_rate"])])
        G.golden_io.save_npz(os.path.join(G.OUT, "sccf_small.npz"), **out)
        size = os.path.getsize(os.path.join(G.OUT, "sccf_small.npz"))
        assert size <= 1 << 20, size
        print("wrote sccf_small.npz (%d bytes)" % size)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
