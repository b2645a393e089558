"""scripts/gen_golden_ncl.py — TEST INFRASTRUCTURE.  Goldens for NCL from the imported reference, on the frozen `small`
inputs (300 users, 250 items) with k = 16 and with the conventions of oracle/gen_golden.py (whose helpers it imports;
nothing under oracle/ changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_ncl.py      # -> tests/golden/ncl_small.npz

The reference module imports faiss at its top; an empty stand-in module of that name is put into sys.modules first.
k-means is never taken from the reference: the clusters of the fixture come from a float64 Lloyd run in this file (initial
centroids: the rows torch.randperm(N, generator=seed 1234)[:k]; 10 iterations; an empty cluster keeps its centroid) on the
model's initial tables, and are set on the reference model under its own attribute names.

For two settings — `def`: the reference's configure/NCL.txt apart from k; `strong`: ssl_lambda = 0.1, proto_lambda = 1e-3,
alpha = 0.6, where the two extra terms dominate the gradient — the loss list and .grad of both tables for a B = 96 batch with
forced duplicate users and items at epoch 0 (three losses) and at epoch 20 (four); the losses and both tables after three
torch.optim.Adam steps on three 256-row batches at epoch 20 with the clusters held fixed; get_rating_for_test for 32 users.
$IDG_GOLDEN_OUT redirects the output directory.
"""
import os
import shutil
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import gen_golden as G  # noqa: E402  (puts the reference first on sys.path and imports it)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.modules.setdefault("faiss", types.ModuleType("faiss"))
from models.NCL import NCL as RefNCL  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

K_CLUSTERS = 16
SETTINGS = {
    "def": {},
    "strong": dict(ssl_lambda=0.1, proto_lambda=1e-3, alpha=0.6),
}


def lloyd64(x, k, niter=10, seed=1234):
    """(centroids float32 [k, d], labels int64 [N]) of a float64 Lloyd run; the labels are nearest-centroid for the
    centroids returned."""
    x = x.astype(np.float64)
    first = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(seed))[:k].numpy()
    c = x[first].copy()

    def nearest(c):
        return ((x * x).sum(1)[:, None] - 2.0 * x @ c.T + (c * c).sum(1)[None, :]).argmin(axis=1)

    for _ in range(niter):
        lab = nearest(c)
        for j in range(k):
            if (lab == j).any():
                c[j] = x[lab == j].mean(axis=0)
    c = c.astype(np.float32)
    return c, nearest(c.astype(np.float64)).astype(np.int64)


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_ncl_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        out = {}
        cfg0 = G.base_config("NCL", dataset=gname, dataset_path=tmp + "/", k=K_CLUSTERS)
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
            cfg = G.base_config("NCL", dataset=gname, dataset_path=tmp + "/", k=K_CLUSTERS, **extra)
            ref_tools.set_seed(G.SEED)
            m = RefNCL(cfg, data, G.CPU)
            # the clusters of the initial tables (the same tables in both settings: one copy in the fixture)
            uc, u2c = lloyd64(m.user_embedding.weight.detach().numpy(), K_CLUSTERS)
            ic, i2c = lloyd64(m.item_embedding.weight.detach().numpy(), K_CLUSTERS)
            if "user_centroids" in out:
                assert np.array_equal(out["user_centroids"], uc) and np.array_equal(out["item_2cluster"], i2c)
            out.update(user_centroids=uc, user_2cluster=u2c, item_centroids=ic, item_2cluster=i2c)
            m.user_centroids, m.user_2cluster = torch.from_numpy(uc), torch.from_numpy(u2c)
            m.item_centroids, m.item_2cluster = torch.from_numpy(ic), torch.from_numpy(i2c)
            for epoch in (0, 20):
                m.zero_grad()
                ll = m(bu, bp, bn, epoch)
                sum(ll).backward()
                out["%s_loss%d" % (tag, epoch)] = np.array([x.item() for x in ll])
                out["%s_grad_user%d" % (tag, epoch)] = m.user_embedding.weight.grad.numpy().copy()
                out["%s_grad_item%d" % (tag, epoch)] = m.item_embedding.weight.grad.numpy().copy()
            with torch.no_grad():
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy()
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj = []
            for i in range(3):
                b = tri3[i * 256:(i + 1) * 256]
                ll = m(b[:, 0], b[:, 1], b[:, 2], 20)
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
            out[tag + "_traj_loss"] = np.array(traj)
            out[tag + "_traj_user"] = m.user_embedding.weight.detach().numpy().copy()
            out[tag + "_traj_item"] = m.item_embedding.weight.detach().numpy().copy()
        G.golden_io.save_npz(os.path.join(G.OUT, "ncl_small.npz"), **out)
        print("wrote ncl_small.npz (%d arrays)" % len(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
