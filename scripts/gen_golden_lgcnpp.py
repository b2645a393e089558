"""scripts/gen_golden_lgcnpp.py — TEST INFRASTRUCTURE.  Goldens for LightGCN++ from the imported reference, on the frozen
`small` inputs (300 users, 250 items; 4 items without a training edge) with the conventions of oracle/gen_golden.py (whose
helpers it imports; nothing under oracle/ changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_lgcnpp.py      # -> tests/golden/lgcnpp_small.npz

For two settings — `def`: the reference's configure/LightGCN_pp.txt (alpha = 0.6, beta = -0.1, gamma = 0.2); `skew`:
alpha = 0.2, beta = 0.9, gamma = 0.5 — the CSR arrays of the adjacency D^-alpha A D^-beta as the reference builds it (a
fresh build: the dataset directory is new), the loss list and .grad of both tables for a B = 96 batch with forced duplicate
users and items, get_rating_for_test for 32 users, and the losses and both tables after three torch.optim.Adam steps on
three 256-row batches.  $IDG_GOLDEN_OUT redirects the output directory.
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

from models.LightGCN_pp import LightGCN_pp as RefLightGCNpp  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

SETTINGS = {
    "def": {},
    "skew": dict(alpha=0.2, beta=0.9, gamma=0.5),
}


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_lgcnpp_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        out = {}
        cfg0 = G.base_config("LightGCN_pp", dataset=gname, dataset_path=tmp + "/")
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
            cfg = G.base_config("LightGCN_pp", dataset=gname, dataset_path=tmp + "/", **extra)
            out[tag + "_abg"] = np.array([float(cfg[k]) for k in ("alpha", "beta", "gamma")])
            ref_tools.set_seed(G.SEED)
            m = RefLightGCNpp(cfg, data, G.CPU)
            A = m.get_sparse_graph()  # the cache file the constructor has just written
            assert A.dtype == np.float32
            out[tag + "_adj_indptr"], out[tag + "_adj_indices"], out[tag + "_adj_data"] = G.csr_arrays(A)
            if tag == "def":
                out["init_user"] = m.user_embedding.weight.detach().numpy().copy()
                out["init_item"] = m.item_embedding.weight.detach().numpy().copy()
            m.zero_grad()
            ll = m(bu, bp, bn)
            sum(ll).backward()
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            out[tag + "_grad_user"] = m.user_embedding.weight.grad.numpy().copy()
            out[tag + "_grad_item"] = m.item_embedding.weight.grad.numpy().copy()
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
        G.golden_io.save_npz(os.path.join(G.OUT, "lgcnpp_small.npz"), **out)
        print("wrote lgcnpp_small.npz (%d arrays)" % len(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
