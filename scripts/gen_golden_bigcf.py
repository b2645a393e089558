"""scripts/gen_golden_bigcf.py — TEST INFRASTRUCTURE.  Goldens for BIGCF from the imported reference, on the frozen `small`
inputs (300 users, 250 items; 4 items without a training edge) with the conventions of oracle/gen_golden.py (whose helpers it
imports; nothing under oracle/ changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_bigcf.py      # -> tests/golden/bigcf_small.npz, bigcf_small_one.npz

The reference ships no configure/BIGCF.txt: the configuration is its LightGCN one plus BIGCF's keys, with this project's
values (configure/BIGCF.txt).  Every torch.randn_like panel the reference draws is RECORDED by a wrapper around it and stored
as float32: with the recorded noise fed back, everything here is deterministic.  A panel is 141 KB and a fixture must stay
below 1 MiB, so torch's generator is re-seeded before every forward — seeds A, B for the loss / gradient forward and the
rating, A, B, A for the three trajectory steps — and the five recorded panels are two distinct ones (asserted), the same in
both settings.  For two settings — `def`: GCN_layer = 2; `one`: GCN_layer = 1 — the initial tables and intent matrices
(the same in both, stored once), the loss list and every .grad for a B = 96 batch with forced duplicate users and items,
get_rating_for_test for 32 users, and the losses and all parameters after three torch.optim.Adam steps on three 256-row
batches.  `def` and everything shared go to bigcf_small.npz, `one` to bigcf_small_one.npz (two files: each below 1 MiB).
$IDG_GOLDEN_OUT redirects the output directory.
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

from models.BIGCF import BIGCF as RefBIGCF  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

BIGCF_KEYS = dict(embedding_size=64, intent_size=128, learn_rate=0.001, reg_lambda=0.0001, ssl_lambda=0.2, ssl_temperature=0.2,
                  int_temperature=1.0, batch_size=2048, test_batch_size=2048)
SETTINGS = {
    "def": dict(GCN_layer=2),
    "one": dict(GCN_layer=1),
}
NOISE_SEEDS = {"a": 7001, "b": 7002}
PARAMS = ("user_embedding", "item_embedding", "user_intent", "item_intent")


class Recorder:
    """torch.randn_like, recording what it returns."""

    def __init__(self):
        self.real, self.panels = torch.randn_like, []

    def __call__(self, *a, **kw):
        z = self.real(*a, **kw)
        self.panels.append(z.detach().clone().numpy().astype(np.float32))
        return z

    def take(self):
        out, self.panels = self.panels, []
        return out


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_bigcf_")
    rec = Recorder()
    torch.randn_like = rec
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        common = dict(dataset=gname, dataset_path=tmp + "/", **BIGCF_KEYS)
        cfg0 = G.base_config("LightGCN", **common, **SETTINGS["def"])
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        shared = {"batch": torch.stack([bu, bp, bn], 1).numpy()}
        tri3 = torch.from_numpy(s1[:3 * 256].copy())
        shared["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        shared["rating_users"] = test_users.numpy()
        files = {}
        for tag, extra in SETTINGS.items():
            out = files[tag] = {}
            cfg = G.base_config("LightGCN", **common, **extra)
            ref_tools.set_seed(G.SEED)
            m = RefBIGCF(cfg, data, G.CPU)
            assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
            prm = {p: getattr(m, p).weight for p in PARAMS}
            for p in PARAMS:
                init = prm[p].detach().numpy().copy()
                if "init_" + p in shared:
                    assert np.array_equal(shared["init_" + p], init)
                shared["init_" + p] = init
            m.zero_grad()
            torch.manual_seed(NOISE_SEEDS["a"])
            ll = m(bu, bp, bn)
            sum(ll).backward()
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            for p in PARAMS:
                out["%s_grad_%s" % (tag, p)] = prm[p].grad.numpy().copy()
            with torch.no_grad():
                torch.manual_seed(NOISE_SEEDS["b"])
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy()
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj = []
            for i in range(3):
                b = tri3[i * 256:(i + 1) * 256]
                torch.manual_seed(NOISE_SEEDS["aba"[i]])
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
            out[tag + "_traj_loss"] = np.array(traj)
            for p in PARAMS:
                out["%s_traj_%s" % (tag, p)] = prm[p].detach().numpy().copy()
            panels = rec.take()  # forward, rating, three steps
            assert len(panels) == 5 and all(z.shape == (data.num_users + data.num_items, 64) for z in panels)
            assert np.array_equal(panels[0], panels[2]) and np.array_equal(panels[0], panels[4]) and np.array_equal(panels[1], panels[3])
            assert not np.array_equal(panels[0], panels[1])
            for name, z in (("noise_a", panels[0]), ("noise_b", panels[1])):
                if name in shared:
                    assert np.array_equal(shared[name], z)
                shared[name] = z
        G.golden_io.save_npz(os.path.join(G.OUT, "bigcf_small.npz"), **shared, **files["def"])
        G.golden_io.save_npz(os.path.join(G.OUT, "bigcf_small_one.npz"), **files["one"])
        for name in ("bigcf_small.npz", "bigcf_small_one.npz"):
            size = os.path.getsize(os.path.join(G.OUT, name))
            assert size <= 1 << 20, (name, size)
            print("wrote %s (%d bytes)" % (name, size))
    finally:
        torch.randn_like = rec.real
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
