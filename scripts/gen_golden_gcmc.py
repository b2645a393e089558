"""scripts/gen_golden_gcmc.py — TEST INFRASTRUCTURE.  Goldens for GCMC from the imported reference, on the frozen `small`
inputs (300 users, 250 items; 4 items without a training edge) with the conventions of oracle/gen_golden.py (whose helpers it
imports; nothing under oracle/ changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_gcmc.py      # -> tests/golden/gcmc_small.npz

mess_drop_prob = [0.0, 0.0, 0.0] throughout: the reference's aggregate() builds nn.Dropout afresh, so message dropout stays
on under .eval() and p = 0 is the only setting in which it is deterministic.  For two settings — `def`: the reference's
configure/GCMC.txt (GCN_layer = 1); `two`: GCN_layer = 2 — the initial W_gcn_l / b_gcn_l / W_mlp_l / b_mlp_l (the two tables
are the same in both and stored once), the loss list and .grad of both tables and of every small tensor for a B = 96 batch
with forced duplicate users and items, get_rating_for_test for 32 users, and the losses and parameters after three
torch.optim.Adam steps on three 256-row batches.  Every tensor is stored whole: the file stays below the 1 MiB a committed
file may have (tests/test_gcmc_host.py holds it to that).  $IDG_GOLDEN_OUT redirects the output directory.
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

from models.GCMC import GCMC as RefGCMC  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

SETTINGS = {
    "def": {},
    "two": dict(GCN_layer=2),
}
NAMES = ("W_gcn_%d", "b_gcn_%d", "W_mlp_%d", "b_mlp_%d")


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_gcmc_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        out = {}
        common = dict(dataset=gname, dataset_path=tmp + "/", mess_drop_prob="[0.0, 0.0, 0.0]")
        cfg0 = G.base_config("GCMC", **common)
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        out["batch"] = torch.stack([bu, bp, bn], 1).numpy()
        tri3 = torch.from_numpy(s1[:3 * 256].copy())
        out["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        out["rating_users"] = test_users.numpy()
        for tag, extra in SETTINGS.items():
            cfg = G.base_config("GCMC", **common, **extra)
            K = int(cfg["GCN_layer"])
            ref_tools.set_seed(G.SEED)
            m = RefGCMC(cfg, data, G.CPU)
            names = [nm % l for l in range(K) for nm in NAMES]
            assert list(m.weight_dict.keys()) == names and len(list(m.parameters())) == 2 + 4 * K
            if tag == "def":
                out["init_user"] = m.user_embedding.weight.detach().numpy().copy()
                out["init_item"] = m.item_embedding.weight.detach().numpy().copy()
            else:
                assert np.array_equal(out["init_user"], m.user_embedding.weight.detach().numpy())
                assert np.array_equal(out["init_item"], m.item_embedding.weight.detach().numpy())
            for nm in names:
                out["%s_%s" % (tag, nm)] = m.weight_dict[nm].detach().numpy().copy()
            m.zero_grad()
            ll = m(bu, bp, bn)
            sum(ll).backward()
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            out[tag + "_grad_user"] = m.user_embedding.weight.grad.numpy().copy()
            out[tag + "_grad_item"] = m.item_embedding.weight.grad.numpy().copy()
            for nm in names:
                out["%s_grad_%s" % (tag, nm)] = m.weight_dict[nm].grad.numpy().copy()
            with torch.no_grad():
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy()
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
            out[tag + "_traj_user"] = m.user_embedding.weight.detach().numpy().copy()
            out[tag + "_traj_item"] = m.item_embedding.weight.detach().numpy().copy()
            for nm in names:
                out["%s_traj_%s" % (tag, nm)] = m.weight_dict[nm].detach().numpy().copy()
        G.golden_io.save_npz(os.path.join(G.OUT, "gcmc_small.npz"), **out)
        print("wrote gcmc_small.npz (%d arrays)" % len(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
