"""scripts/gen_golden_cvga.py — TEST INFRASTRUCTURE.  Goldens for CVGA from the imported reference, on the frozen
`small` inputs and with the conventions of oracle/gen_golden.py (whose helpers it imports; nothing under oracle/
changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_cvga.py      # -> tests/golden/cvga_small.npz

With dropout = 0, and eps recorded by wrapping torch.randn_like during the reference's calls (its encoder draws eps for
every user; the batch's rows are kept): the initial four tensors; for one batch of 96 users the loss pair and the four
.grad; three torch.optim.Adam steps on the first three 96-user batches of the reference trainer's shuffled order, with
the losses and the four tensors after each step; get_rating_for_test for 32 users; get_ELBO_loss values and input
gradients on a B = 1 and a B = 2 block.  $IDG_GOLDEN_OUT redirects the output directory.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_cvga.py --curve   # -> tests/golden/cvga_curve_medium.npz

The reference's own CVGA_trainer, three seeds, on the frozen medium_conv inputs (tests/golden/inputs/medium_conv/, the
dataset of oracle/gen_golden_convergence.py) with configure/CVGA.txt's dropout 0.3, learn_rate and batch_size, 31 epochs,
interval 5, one CPU thread: every epoch's logged loss triple (total, recon, KL) and Recall / NDCG @[20, 40] at every
tested epoch — the reference's own run-to-run spread (~90 s).
"""
import io
import logging
import os
import re
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import gen_golden as G  # noqa: E402  (puts the reference first on sys.path and imports it)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from models.CVGA import CVGA as RefCVGA  # noqa: E402

ref_tools, ref_loader, ref_losses = G.ref_tools, G.ref_loader, G.ref_losses
NAMES = ("wq", "bq", "wp", "c")
B = 96


class _RecordEps:
    """torch.randn_like, recorded: the reference's reparameterize draws through it (models/CVGA.py:65)."""

    def __init__(self):
        self.draws = []
        self._orig = torch.randn_like

    def __enter__(self):
        def wrapped(*a, **kw):
            t = self._orig(*a, **kw)
            self.draws.append(t.detach().clone())
            return t

        torch.randn_like = wrapped
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._orig


def _tensors(m):
    return [m.q_layers[0].weight, m.q_layers[0].bias, m.p_layers[0].weight, m.p_layers[0].bias]


def _x(data, users):
    return torch.FloatTensor(data.user_item_net[users.numpy()].toarray())


def _loss_blocks(out):
    gen = torch.Generator().manual_seed(G.SEED)
    for nb in (1, 2):
        r = torch.randn(nb, 12, generator=gen) * 2
        x = torch.zeros(nb, 12)
        x[:, 1], x[0, 5], x[-1, 7] = 1.0, 2.0, 1.0
        mu, lv = torch.randn(nb, 4, generator=gen), torch.randn(nb, 4, generator=gen) * 0.5
        out["blk%d_recon_x" % nb], out["blk%d_x" % nb] = r.numpy().copy(), x.numpy().copy()
        out["blk%d_mu" % nb], out["blk%d_logvar" % nb] = mu.numpy().copy(), lv.numpy().copy()
        rr, mr, lr = (t.clone().requires_grad_(True) for t in (r, mu, lv))
        bce, kld = ref_losses.get_ELBO_loss(rr, x, mr, lr, 1.0)
        (bce + kld).backward()
        out["blk%d_bce" % nb], out["blk%d_kld" % nb] = np.array(bce.item()), np.array(kld.item())
        out["blk%d_g_recon" % nb] = rr.grad.numpy().copy()
        out["blk%d_g_mu" % nb], out["blk%d_g_logvar" % nb] = mr.grad.numpy().copy(), lr.grad.numpy().copy()


CURVE_SEEDS, CURVE_EPOCHS, CURVE_INTERVAL = (2024, 2025, 2026), 31, 5


def _numbers(text):
    return [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?", text)]


def curve():
    """The three-seed learning curves of the reference trainer on medium_conv (cvga_curve_medium.npz)."""
    from models.CVGA import Trainer as RefTrainer

    torch.set_num_threads(1)
    tmp = tempfile.mkdtemp(prefix="idg_golden_cvga_curve_")
    try:
        def draw(d):  # (not reached: the frozen files exist; oracle/gen_golden_convergence.py's draw)
            U, I, E = G.synth.SHAPES["medium"]
            users, items = G.synth.generate(U, I, E, seed=11)
            (tu, ti), (su, si) = G.synth.split_test(users, items, U, n_test=5, seed=12)
            G.synth.write_ratings(os.path.join(d, "train.txt"), tu, ti)
            G.synth.write_ratings(os.path.join(d, "test.txt"), su, si)

        path = G.golden_io.frozen_dataset("medium_conv", os.path.join(tmp, "medium"), draw)
        cfg = G.base_config("CVGA", dataset="medium", dataset_path=tmp + "/", training_epochs=CURVE_EPOCHS,
                            interval=CURVE_INTERVAL, early_stopping=1000)
        losses, recall, ndcg, epochs = [], [], [], None
        for seed in CURVE_SEEDS:
            stream = io.StringIO()
            logger = logging.getLogger("golden_cvga_curve_%d" % seed)
            logger.setLevel(logging.INFO)
            logger.handlers = [logging.StreamHandler(stream)]
            ref_tools.set_seed(seed)
            data = ref_loader.Data(path, cfg)
            RefTrainer(None, cfg, data, G.CPU, logger).train()
            lines = stream.getvalue().splitlines()
            losses.append([_numbers(ln.split("training loss:")[1]) for ln in lines if "training loss" in ln])
            tests = [ln for ln in lines if "Test recall" in ln]
            epochs = [int(_numbers(ln.split("|")[0])[0]) for ln in tests]
            recall.append([_numbers(ln.split("Test recall:")[1].split("|")[0]) for ln in tests])
            ndcg.append([_numbers(ln.split("Test NDCG:")[1]) for ln in tests])
        out = {"seeds": np.array(CURVE_SEEDS, dtype=np.int64), "loss": np.array(losses), "test_epochs": np.array(epochs),
               "recall": np.array(recall), "ndcg": np.array(ndcg), "top_k": np.array(eval(cfg["top_K"]), dtype=np.int64),
               "config_keys": np.array(sorted(cfg)),
               "config_values": np.array([dict(cfg, dataset_path="<tmp>/")[k] for k in sorted(cfg)])}
        G.golden_io.save_npz(os.path.join(G.OUT, "cvga_curve_medium.npz"), **out)
        print("wrote cvga_curve_medium.npz: recall@20 per seed", out["recall"][:, :, 0].tolist())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_cvga_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        out = {}
        cfg = G.base_config("CVGA", dataset=gname, dataset_path=tmp + "/", dropout=0, batch_size=B)
        ref_tools.set_seed(G.SEED)
        data = ref_loader.Data(path, cfg)
        ref_tools.set_seed(G.SEED)
        m = RefCVGA(cfg, data, G.CPU)
        for name, t in zip(NAMES, _tensors(m)):
            out["init_" + name] = t.detach().numpy().copy()
        # one batch: the loss pair and the four gradients
        users = torch.arange(7, 7 + 3 * B, 3)
        out["batch_users"] = users.numpy()
        m.zero_grad()
        with _RecordEps() as rec:
            ll = m(users, _x(data, users))
        out["batch_eps"] = rec.draws[0][users].numpy().copy()
        sum(ll).backward()
        out["batch_loss"] = np.array([x.item() for x in ll])
        for name, t in zip(NAMES, _tensors(m)):
            out["grad_" + name] = t.grad.numpy().copy()
        # get_rating_for_test on the initial model (eval: no dropout anyway at p = 0)
        m.eval()
        rusers = torch.from_numpy(np.array(list(data.test_dict.keys()))[:32])
        out["rating_users"] = rusers.numpy()
        with torch.no_grad(), _RecordEps() as rec:
            out["rating"] = m.get_rating_for_test(rusers).numpy()
        out["rating_eps"] = rec.draws[0][rusers].numpy().copy()
        m.train()
        # three Adam steps on the trainer's first three batches (models/CVGA.py:104-150)
        ref_tools.set_seed(G.SEED)
        m = RefCVGA(cfg, data, G.CPU)
        opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
        user_list = list(range(data.num_users))
        np.random.shuffle(user_list)
        out["order"] = np.array(user_list, dtype=np.int64)
        losses, eps = [], []
        for step in range(3):
            bu = torch.Tensor(user_list[step * B:(step + 1) * B]).long()
            with _RecordEps() as rec:
                ll = m(bu, _x(data, bu))
            eps.append(rec.draws[0][bu].numpy().copy())
            losses.append([x.item() for x in ll])
            opt.zero_grad()
            sum(ll).backward()
            opt.step()
            for name, t in zip(NAMES, _tensors(m)):
                out["traj%d_%s" % (step, name)] = t.detach().numpy().copy()
        out["traj_loss"], out["traj_eps"] = np.array(losses), np.stack(eps)
        _loss_blocks(out)
        G.golden_io.save_npz(os.path.join(G.OUT, "cvga_small.npz"), **out)
        print("wrote cvga_small.npz (%d arrays)" % len(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    curve() if "--curve" in sys.argv else main()
