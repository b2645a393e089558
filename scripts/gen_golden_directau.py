"""scripts/gen_golden_directau.py — TEST INFRASTRUCTURE.  Goldens for DirectAU from the imported reference, on the
frozen `small` inputs and with the conventions of oracle/gen_golden.py (whose helpers it imports; nothing under oracle/
changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_directau.py      # -> tests/golden/directau_small.npz

For both encoders (LightGCN, MF): the loss triple and .grad of both tables for a B = 96 batch with forced duplicate users
and items; the loss triples and both tables after three torch.optim.Adam steps on three 256-row batches;
get_rating_for_test for 32 users.  And the loss functions alone on a B = 1 and a B = 2 block (values and gradients).
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
from models.DirectAU import DirectAU as RefDirectAU  # noqa: E402

ref_tools, ref_loader, ref_losses = G.ref_tools, G.ref_loader, G.ref_losses


def _loss_blocks(out):
    """get_align_loss / get_uniform_loss on a one-row and a two-row block: values and input gradients."""
    gen = torch.Generator().manual_seed(G.SEED)
    for B in (1, 2):
        x = torch.randn(B, 8, generator=gen, dtype=torch.float32)
        y = torch.randn(B, 8, generator=gen, dtype=torch.float32)
        out["blk%d_x" % B], out["blk%d_y" % B] = x.numpy().copy(), y.numpy().copy()
        xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        a = ref_losses.get_align_loss(xr, yr)
        a.backward()
        out["blk%d_align" % B] = np.array(a.item())
        out["blk%d_align_gx" % B], out["blk%d_align_gy" % B] = xr.grad.numpy().copy(), yr.grad.numpy().copy()
        xr = x.clone().requires_grad_(True)
        u = ref_losses.get_uniform_loss(xr)
        u.backward()
        out["blk%d_uniform" % B] = np.array(u.item())
        out["blk%d_uniform_gx" % B] = xr.grad.numpy().copy()


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_directau_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        out = {}
        cfg0 = G.base_config("DirectAU", dataset=gname, dataset_path=tmp + "/")
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
        for enc in ("LightGCN", "MF"):
            tag = enc.lower()
            cfg = G.base_config("DirectAU", dataset=gname, dataset_path=tmp + "/", encoder=enc)
            ref_tools.set_seed(G.SEED)
            m = RefDirectAU(cfg, data, G.CPU)
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
        _loss_blocks(out)
        G.golden_io.save_npz(os.path.join(G.OUT, "directau_small.npz"), **out)
        print("wrote directau_small.npz (%d arrays)" % len(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
