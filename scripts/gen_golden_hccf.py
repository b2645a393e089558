"""scripts/gen_golden_hccf.py — TEST INFRASTRUCTURE.  Goldens for HCCF from the imported reference, on the frozen `small`
inputs (300 users, 250 items) with the conventions of oracle/gen_golden.py (whose helpers it imports; nothing under oracle/
changes).  Runs only where the reference exists, on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_hccf.py      # -> tests/golden/hccf_small.npz, hccf_small_drop.npz

Two settings — `def`: the reference's configure/HCCF.txt (keeprate = 1.0, GCN_layer = 3); `drop`: keeprate = 0.5,
GCN_layer = 2.  The four tables are initialised in float32, as the reference does; the model (and its adjacency) is then
cast to float64 and the reference's own forward, backward and torch.optim.Adam run in float64, so the fixture carries no
float32 rounding of the reference's; gradients, tables and ratings are stored rounded to float32, the losses as float64.

Every keep mask the reference draws is RECORDED: the name `F` of the imported reference module is pointed at a stand-in
whose dropout() calls the real one and keeps mask = (y != 0) | (x == 0) (an element that is zero before the dropout counts
as kept: it is zero either way).  A forward draws 2 * GCN_layer masks — per layer the users' [300, 64], then the items'
[250, 64] — and so does get_rating_for_test (the reference's F.dropout has no training= argument).  At `def` every mask is
all ones (asserted, not stored); at `drop` they are stored bit-packed along the hyperedge axis, [.., GCN_layer, 550, 8].

Stored: the initial tables (the same in both settings, stored once), a B = 96 batch with forced duplicate users and items,
the three losses and all four .grad, get_rating_for_test for 32 users, and the losses and the four tensors after three
torch.optim.Adam steps on three 256-row batches.  `def` and everything shared go to hccf_small.npz, `drop` to
hccf_small_drop.npz (two files: each below 1 MiB).  $IDG_GOLDEN_OUT redirects the output directory.
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

import models.HCCF as ref_hccf  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

SETTINGS = {
    "def": dict(keeprate=1.0, GCN_layer=3),
    "drop": dict(keeprate=0.5, GCN_layer=2),
}
FILES = {"def": "hccf_small.npz", "drop": "hccf_small_drop.npz"}
PARAMS = ("user_embedding", "item_embedding", "user_hyper_emb", "item_hyper_emb")


class RecordingF:
    """Stands in for torch.nn.functional inside the reference module: dropout() records its keep mask."""

    def __init__(self, real):
        self.real, self.masks = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def dropout(self, x, *a, **kw):
        y = self.real.dropout(x, *a, **kw)
        self.masks.append(((y != 0) | (x == 0)).detach().numpy().copy())
        return y

    def take(self):
        out, self.masks = self.masks, []
        return out


def pack(masks, K, U, I):
    """2 K masks of one forward (users', items' per layer) -> uint8 [K, U + I, 8]."""
    assert len(masks) == 2 * K and all(m.shape == ((U, I)[j & 1], 64) for j, m in enumerate(masks))
    return np.stack([np.packbits(np.concatenate(masks[2 * l:2 * l + 2]), axis=1) for l in range(K)])


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_hccf_")
    rec = RecordingF(ref_hccf.F)
    ref_hccf.F = rec
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        cfg0 = G.base_config("HCCF", dataset=gname, dataset_path=tmp + "/")
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg0)
        U, I = data.num_users, data.num_items
        np.random.seed(G.SEED)
        s1 = data.sample_data_to_train_all()
        B = 96
        bu, bp, bn = (torch.from_numpy(s1[:B, c].copy()) for c in range(3))
        bu[1], bp[1], bu[5], bp[7] = bu[0], bp[0], bu[3], bp[2]  # duplicate users and items inside the batch
        assert int(torch.unique(bu).numel()) < B and int(torch.unique(bp).numel()) < B
        shared = {"batch": torch.stack([bu, bp, bn], 1).numpy()}
        tri3 = torch.from_numpy(s1[:3 * 256].copy())
        shared["traj_batches"] = tri3.numpy()
        test_users = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        shared["rating_users"] = test_users.numpy()
        files = {}
        for tag, extra in SETTINGS.items():
            out = files[tag] = {}
            K = extra["GCN_layer"]
            cfg = G.base_config("HCCF", dataset=gname, dataset_path=tmp + "/", **extra)
            ref_tools.set_seed(G.SEED)
            m = ref_hccf.HCCF(cfg, data, G.CPU)
            assert [n for n, _ in m.named_parameters()] == [p + ".weight" for p in PARAMS]
            for p in PARAMS:
                init = getattr(m, p).weight.detach().numpy().copy()
                if "init_" + p in shared:
                    assert np.array_equal(shared["init_" + p], init)
                shared["init_" + p] = init
            # the float32 initial values, then the reference's own program in float64
            m = m.double()
            m.Graph = m.Graph.double()
            prm = {p: getattr(m, p).weight for p in PARAMS}
            m.zero_grad()
            ll = m(bu, bp, bn)
            assert len(ll) == 3
            sum(ll).backward()
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            for p in PARAMS:
                out["%s_grad_%s" % (tag, p)] = prm[p].grad.numpy().astype(np.float32)
            masks = {"fwd": pack(rec.take(), K, U, I)}
            with torch.no_grad():
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy().astype(np.float32)
            masks["rating"] = pack(rec.take(), K, U, I)
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj, tmasks = [], []
            for i in range(3):
                b = tri3[i * 256:(i + 1) * 256]
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
                tmasks.append(pack(rec.take(), K, U, I))
            masks["traj"] = np.stack(tmasks)
            out[tag + "_traj_loss"] = np.array(traj)
            for p in PARAMS:
                out["%s_traj_%s" % (tag, p)] = prm[p].detach().numpy().astype(np.float32)
            if extra["keeprate"] >= 1.0:
                assert all(bool((v == 255).all()) for v in masks.values())
            else:
                assert not np.array_equal(masks["fwd"][0], masks["fwd"][1]) and not np.array_equal(masks["fwd"], masks["rating"])
                for name, v in masks.items():
                    out["%s_masks_%s" % (tag, name)] = v
            out[tag + "_hyper"] = np.array([extra["keeprate"], K, float(cfg["learn_rate"]), float(cfg["reg_lambda"]),
                                            float(cfg["ssl_lambda"]), float(cfg["temperature"])])
        G.golden_io.save_npz(os.path.join(G.OUT, FILES["def"]), **shared, **files["def"])
        G.golden_io.save_npz(os.path.join(G.OUT, FILES["drop"]), **files["drop"])
        for name in FILES.values():
            size = os.path.getsize(os.path.join(G.OUT, name))
            assert size <= 1 << 20, (name, size)
            print("wrote %s (%d bytes)" % (name, size))
    finally:
        ref_hccf.F = rec.real
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
