"""scripts/gen_golden_lightgcl.py — TEST INFRASTRUCTURE.  Goldens for LightGCL from the imported reference, on the frozen `small`
inputs (300 users, 250 items) with the conventions of oracle/gen_golden.py (whose helpers it imports; nothing under oracle/
changes).  Runs only where the reference exists, on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_lightgcl.py      # -> tests/golden/lightgcl_small.npz

The reference's constructor draws its tables and its truncated SVD (torch.svd_lowrank of the rectangular normalised
adjacency) in float32; torch.svd_lowrank is wrapped to RECORD the factors (svd_u, s, svd_v) it returns.  The model is then cast
to float64 — tables, adjacency, and the four factor products rebuilt in float64 from the recorded float32 factors, which the
reference keeps as plain attributes — and the reference's own forward, backward and torch.optim.Adam run in float64, so the
fixture carries no float32 rounding of the reference's arithmetic.  Everything is stored as float64 (the gradients too: the
host test holds the float64 statement to them at 1e-10), except the factors and initial tables, which ARE float32 values.

Two settings.  `def`: this project's configure/LightGCL.txt values (GCN_layer = 2, svd_q = 5, temperature = 0.2) at
embedding_size = 32, the narrowest width the fused step is built for (the file stays below mixrec_small.npz).  `clamp`:
GCN_layer = 3, svd_q = 3 and the initial tables scaled by CLAMP_SCALE, so that the clamp of the positive term is active: asserted
below, between 20 % and 80 % of the batch's rows on each side have an unclamped positive outside [-5, 5], and none lies within
1e-3 of +-5 (the gradient jumps there).  Stored: the rectangular adjacency the reference's model holds (float32 CSR), and per setting the factors, the initial tables, the three losses and both .grad
of a B = 96 batch with forced duplicate users and items, the unclamped positives of both sides, the rating of 32 users, the
losses of three torch.optim.Adam steps on three 128-row batches and the tables after the third.  $IDG_GOLDEN_OUT redirects the output directory.
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

from models.LightGCL import LightGCL as RefLightGCL  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

COMMON = dict(embedding_size=32, batch_size=2048, test_batch_size=2048, learn_rate=0.001, reg_lambda=1e-6, ssl_lambda=0.5)
SETTINGS = {
    "def": dict(GCN_layer=2, svd_q=5, temperature=0.2),
    "clamp": dict(GCN_layer=3, svd_q=3, temperature=0.2),
}
CLAMP_SCALE = 2.085  # the xavier tables of the `small` inputs give positives of 0.6 .. 2.6; times 2.085^2 they straddle 5
PARAMS = ("user_embedding", "item_embedding")


def positives(m, users, pos, tau):
    with torch.no_grad():
        fu, fi, gu, gi = m.aggregate()
        return (fu[users] * gu[users]).sum(1) / tau, (fi[pos] * gi[pos]).sum(1) / tau


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_lightgcl_")
    real_svd = torch.svd_lowrank
    recorded = []

    def rec_svd(*a, **kw):
        out = real_svd(*a, **kw)
        recorded.append(tuple(t.detach().clone() for t in out))
        return out

    torch.svd_lowrank = rec_svd
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        cfg0 = G.base_config("LightGCN", dataset=gname, dataset_path=tmp + "/", **COMMON, **SETTINGS["def"])
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        s1 = s1[np.random.RandomState(G.SEED).permutation(len(s1))]  # the sampler's rows come user by user: mix the users
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        out = {"batch": torch.stack([bu, bp, bn], 1).numpy()}
        tri3 = torch.from_numpy(s1[B:B + 3 * 128].copy())
        out["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        out["rating_users"] = test_users.numpy()
        # the rectangular normalised adjacency as the reference's model holds it (float32 values, CSR order): the symmetric
        # adjacency of graph_small.npz carries the same entries rounded along another route, a last place apart
        Rm = G.ref_graph.sparse_adjacency_matrix_R(data).tocsr().astype(np.float32)
        Rm.sort_indices()
        out["R_indptr"], out["R_indices"], out["R_data"] = Rm.indptr.astype(np.int64), Rm.indices.astype(np.int32), Rm.data
        for tag, extra in SETTINGS.items():
            cfg = G.base_config("LightGCN", dataset=gname, dataset_path=tmp + "/", **COMMON, **extra)
            tau = float(extra["temperature"])
            ref_tools.set_seed(G.SEED)
            del recorded[:]
            m = RefLightGCL(cfg, data, G.CPU)
            assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
            assert len(recorded) == 1
            svd_u, s, svd_v = recorded[0]
            assert svd_u.dtype == torch.float32 and svd_u.shape == (data.num_users, extra["svd_q"]) and s.shape == (extra["svd_q"],)
            out[tag + "_svd_u"], out[tag + "_s"], out[tag + "_svd_v"] = svd_u.numpy(), s.numpy(), svd_v.numpy()
            if tag == "clamp":
                with torch.no_grad():
                    for p in PARAMS:
                        getattr(m, p).weight.mul_(CLAMP_SCALE)
            for p in PARAMS:
                out["%s_init_%s" % (tag, p)] = getattr(m, p).weight.detach().numpy().copy()
            # the float32 inputs, then the reference's own program in float64
            m = m.double()
            m.Graph = m.Graph.double()
            u64, s64, v64 = svd_u.double(), s.double(), svd_v.double()
            m.u_T, m.v_T = u64.T, v64.T
            m.u_mul_s, m.v_mul_s = u64 @ torch.diag(s64), v64 @ torch.diag(s64)
            prm = {p: getattr(m, p).weight for p in PARAMS}
            pu, pi = positives(m, bu, bp, tau)
            out[tag + "_pos_u"], out[tag + "_pos_i"] = pu.numpy(), pi.numpy()
            if tag == "clamp":
                for side in (pu, pi):
                    share = float((side.abs() > 5).double().mean())
                    assert 0.2 <= share <= 0.8, share
                    assert float((side.abs() - 5).abs().min()) > 1e-3
            else:
                assert float(pu.abs().max()) < 5 and float(pi.abs().max()) < 5
            m.zero_grad()
            ll = m(bu, bp, bn)
            assert len(ll) == 3
            sum(ll).backward()
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            for p in PARAMS:
                out["%s_grad_%s" % (tag, p)] = prm[p].grad.numpy().copy()
            with torch.no_grad():
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy().astype(np.float32)
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj = []
            for i in range(3):
                b = tri3[i * 128:(i + 1) * 128]
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
            out[tag + "_traj_loss"] = np.array(traj)
            for p in PARAMS:
                out["%s_traj_%s" % (tag, p)] = prm[p].detach().numpy().astype(np.float32)
            out[tag + "_hyper"] = np.array([COMMON["reg_lambda"], COMMON["ssl_lambda"], tau, extra["GCN_layer"], extra["svd_q"],
                                            COMMON["learn_rate"]])
        out["clamp_scale"] = np.array([CLAMP_SCALE])
        G.golden_io.save_npz(os.path.join(G.OUT, "lightgcl_small.npz"), **out)
        size = os.path.getsize(os.path.join(G.OUT, "lightgcl_small.npz"))
        assert size <= 706582, size  # tests/golden/mixrec_small.npz
        print("wrote lightgcl_small.npz (%d bytes)" % size)
    finally:
        torch.svd_lowrank = real_svd
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
