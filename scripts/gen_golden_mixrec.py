"""scripts/gen_golden_mixrec.py — TEST INFRASTRUCTURE.  Goldens for MixRec from the imported reference, on the frozen `small`
inputs (300 users, 250 items; 4 items without a training edge) with the conventions of oracle/gen_golden.py (whose helpers it
imports; nothing under oracle/ changes).  Runs only where the reference exists, on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_mixrec.py      # -> tests/golden/mixrec_small.npz

The reference's forward() calls .cuda() on its two permutations: inside this process torch.Tensor.cuda is the identity.
np.random.beta, np.random.dirichlet and torch.randperm are wrapped to RECORD every draw; numpy's and torch's generators are
seeded before every forward (DRAW_SEEDS), so idgrec_amd.mixrec.draw_mix under the same seeds must return the same draws.  Two
settings — `def`: this project's configure/MixRec.txt values with GCN_layer = 2; `mid`: alpha = beta = 2, gamma = 1, where both
Beta draws are asserted to lie in [0.2, 0.8] (at 0.1 / 0.1 the draw is U-shaped and one half of every term can carry almost
no weight, which would hide a wrong half).  The tables are initialised in float32, as the reference does; the model (and
its adjacency) is then cast to float64 and the reference's own forward, backward and torch.optim.Adam run in float64, so the
fixture carries no float32 rounding of the reference's (its float32 gradients sit 6.7e-6 of their largest entry from these);
gradients, tables and ratings are stored rounded to float32, the losses as float64.  Stored: the initial tables (the same in
both settings, stored once), a B = 96 batch with forced duplicate users and items and one negative without a training edge,
the recorded draws, the four losses and both .grad, get_rating_for_test for 32 users, and the losses and tables after three
torch.optim.Adam steps on three 256-row batches with their draws.  $IDG_GOLDEN_OUT redirects the output directory.
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

from models.MixRec import MixRec as RefMixRec  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

MIXREC_KEYS = dict(embedding_size=64, batch_size=2048, test_batch_size=2048, learn_rate=0.001, reg_lambda=0.0001, GCN_layer=2,
                   ssl_lambda=1.1, temperature=0.2)
SETTINGS = {
    "def": dict(alpha=0.1, beta=0.1, gamma=0.1),
    "mid": dict(alpha=2.0, beta=2.0, gamma=1.0),
}
DRAW_SEEDS = {"grad": 8115, "traj": (8128, 8130, 8144)}  # chosen so that `mid`'s assertion below holds in all four forwards
PARAMS = ("user_embedding", "item_embedding")


class Recorder:
    """np.random.beta, np.random.dirichlet and torch.randperm, recording what they return."""

    def __init__(self):
        self.real = (np.random.beta, np.random.dirichlet, torch.randperm, torch.Tensor.cuda)
        self.betas, self.nus, self.perms = [], [], []

    def install(self):
        beta, dirichlet, randperm, _ = self.real

        def rec_beta(*a, **kw):
            v = beta(*a, **kw)
            self.betas.append(float(v))
            return v

        def rec_dirichlet(*a, **kw):
            v = dirichlet(*a, **kw)
            self.nus.append(np.asarray(v, dtype=np.float64).reshape(-1).copy())
            return v

        def rec_randperm(*a, **kw):
            v = randperm(*a, **kw)
            self.perms.append(v.numpy().copy())
            return v

        np.random.beta, np.random.dirichlet, torch.randperm = rec_beta, rec_dirichlet, rec_randperm
        torch.Tensor.cuda = lambda self, *a, **kw: self

    def remove(self):
        np.random.beta, np.random.dirichlet, torch.randperm, torch.Tensor.cuda = self.real

    def take(self):
        """(user_beta, item_beta, nu float32 [B], user_perm, item_perm) of the one forward since the last take()."""
        assert len(self.betas) == 2 and len(self.nus) == 1 and len(self.perms) == 2, (len(self.betas), len(self.nus), len(self.perms))
        out = (np.array(self.betas, dtype=np.float64), torch.FloatTensor(self.nus[0]).numpy().copy(), self.perms[0], self.perms[1])
        self.betas, self.nus, self.perms = [], [], []
        return out


def seed_draws(seed):
    np.random.seed(seed)
    torch.manual_seed(seed)


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_mixrec_")
    rec = Recorder()
    rec.install()
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        common = dict(dataset=gname, dataset_path=tmp + "/", **MIXREC_KEYS)
        cfg0 = G.base_config("LightGCN", **common, **SETTINGS["def"])
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        cold = np.setdiff1d(np.arange(data.num_items), np.unique(np.asarray(data.train_item)))
        assert cold.size >= 1
        bn[9] = int(cold[0])  # a negative without a training edge: its propagated row is zero
        out = {"batch": torch.stack([bu, bp, bn], 1).numpy(), "cold_item": np.array([cold[0]], dtype=np.int64)}
        tri3 = torch.from_numpy(s1[:3 * 256].copy())
        out["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        out["rating_users"] = test_users.numpy()
        for tag, extra in SETTINGS.items():
            cfg = G.base_config("LightGCN", **common, **extra)
            ref_tools.set_seed(G.SEED)
            m = RefMixRec(cfg, data, G.CPU)
            assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
            prm = {p: getattr(m, p).weight for p in PARAMS}
            for p in PARAMS:
                init = prm[p].detach().numpy().copy()
                if "init_" + p in out:
                    assert np.array_equal(out["init_" + p], init)
                out["init_" + p] = init
            # the float32 initial values, then the reference's own program in float64
            m = m.double()
            m.Graph = m.Graph.double()
            prm = {p: getattr(m, p).weight for p in PARAMS}
            m.zero_grad()
            seed_draws(DRAW_SEEDS["grad"])
            ll = m(bu, bp, bn)
            sum(ll).backward()
            assert len(ll) == 4
            betas, nu, uperm, iperm = rec.take()
            if tag == "mid":
                assert np.all((betas >= 0.2) & (betas <= 0.8)), betas
            out[tag + "_betas"], out[tag + "_nu"], out[tag + "_user_perm"], out[tag + "_item_perm"] = betas, nu, uperm, iperm
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            for p in PARAMS:
                out["%s_grad_%s" % (tag, p)] = prm[p].grad.numpy().astype(np.float32)
            with torch.no_grad():
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy().astype(np.float32)
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj = []
            for i in range(3):
                b = tri3[i * 256:(i + 1) * 256]
                seed_draws(DRAW_SEEDS["traj"][i])
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
                betas, nu, uperm, iperm = rec.take()
                if tag == "mid":
                    assert np.all((betas >= 0.2) & (betas <= 0.8)), betas
                out["%s_traj%d_betas" % (tag, i)], out["%s_traj%d_nu" % (tag, i)] = betas, nu
                out["%s_traj%d_user_perm" % (tag, i)], out["%s_traj%d_item_perm" % (tag, i)] = uperm, iperm
            out[tag + "_traj_loss"] = np.array(traj)
            for p in PARAMS:
                out["%s_traj_%s" % (tag, p)] = prm[p].detach().numpy().astype(np.float32)
        out["draw_seeds"] = np.array([DRAW_SEEDS["grad"], *DRAW_SEEDS["traj"]], dtype=np.int64)
        for tag, extra in SETTINGS.items():
            out[tag + "_abg"] = np.array([extra["alpha"], extra["beta"], extra["gamma"]])
        out["hyper"] = np.array([MIXREC_KEYS["reg_lambda"], MIXREC_KEYS["ssl_lambda"], MIXREC_KEYS["temperature"],
                                 MIXREC_KEYS["GCN_layer"], MIXREC_KEYS["learn_rate"]])
        G.golden_io.save_npz(os.path.join(G.OUT, "mixrec_small.npz"), **out)
        size = os.path.getsize(os.path.join(G.OUT, "mixrec_small.npz"))
        assert size <= 1 << 20, size
        print("wrote mixrec_small.npz (%d bytes)" % size)
    finally:
        rec.remove()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
