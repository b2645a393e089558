"""scripts/gen_golden_impgcn.py — TEST INFRASTRUCTURE.  Goldens for IMP-GCN from the imported reference, on the frozen `small`
inputs (300 users, 250 items; 4 items without a training edge) with the conventions of oracle/gen_golden.py (whose helpers it
imports; nothing under oracle/ changes).  Runs only where the reference exists.

    PYTHONDONTWRITEBYTECODE=1 python -B scripts/gen_golden_impgcn.py      # -> tests/golden/impgcn_small.npz

Two settings — `def`: the reference's configure/IMPGCN.txt (group = 3, GCN_layer = 6); `two`: group = 2, GCN_layer = 3.  The
two tables and fc are the same in both (one seed, one creation order) and stored once; fc_group per setting.

The membership is a local of the reference's aggregate(): it is recorded from the `group` argument of its own get_subgraph
calls (one row of the [num_group, num_nodes] matrix per group).

Evaluation mode (.eval(): both dropouts off): the reference's membership, the `final` panels, get_rating_for_test for 32
users.  Training mode: the reference's self.dropout is replaced by a stand-in whose k-th call multiplies by the k-th PUBLISHED
mask (tests/ngcf_ref64.keep_mask, p = 0.4, one seed, the given stream ids) — the masks the library's kernel regenerates — and
the loss list and .grad of both tables are recorded for a B = 96 batch with forced duplicate users and items, together with
the membership, whether .grad of the four fc tensors is None, and the losses, memberships and tables after three
torch.optim.Adam steps on three 256-row batches (and that the four fc tensors did not move).  The file stays below the 1 MiB
a committed file may have (tests/test_impgcn_host.py holds it to that).  $IDG_GOLDEN_OUT redirects the output directory.
"""
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402  (puts the reference first on sys.path and imports it)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.IMPGCN import IMPGCN as RefIMPGCN  # noqa: E402

sys.path.append(ROOT)  # LAST: `utility` and `models` keep resolving to the reference, `tests` is this repository's
from tests.ngcf_ref64 import keep_mask  # noqa: E402

ref_tools, ref_loader = G.ref_tools, G.ref_loader

SETTINGS = {
    "def": {},
    "two": dict(group=2, GCN_layer=3),
}
P_DROP = 0.4
MASK_SEED = 20241019
GRAD_STREAMS = (3, 4)                       # the B = 96 batch: first and second mask
TRAJ_STREAMS = ((11, 12), (13, 14), (15, 16))  # the three Adam steps


class PublishedDropout(torch.nn.Module):
    """Stands where the reference's nn.Dropout(p = 0.4) stands: call k multiplies by the published mask of streams[k]."""

    def __init__(self, streams):
        super().__init__()
        self.streams, self.calls = list(streams), 0

    def forward(self, x):
        mask = keep_mask(P_DROP, MASK_SEED, self.streams[self.calls], x.shape[0], x.shape[1], dtype=torch.float32)
        self.calls += 1
        return x * mask


def record_membership(model):
    """Wrap the reference's get_subgraph: the rows of its [num_group, num_nodes] membership arrive as `group`, dim 1 first."""
    seen = []
    inner = model.get_subgraph

    def get_subgraph(graph, group, dim):
        if dim == 1:
            seen.append(group.detach().clone())
        return inner(graph, group, dim)

    model.get_subgraph = get_subgraph
    return seen


def member_bytes(seen, groups):
    rows = torch.stack(seen[-groups:])  # [G, n] of 0. / 1.
    assert set(rows.unique().tolist()) <= {0.0, 1.0}
    return sum((rows[g].to(torch.int64) << g) for g in range(groups)).to(torch.uint8).numpy()


def main():
    tmp = tempfile.mkdtemp(prefix="idg_golden_impgcn_")
    try:
        gname = "small"
        path = G.make_data(tmp, gname)
        out = {}
        common = dict(dataset=gname, dataset_path=tmp + "/")
        cfg0 = G.base_config("IMPGCN", **common)
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
        out["mask_seed"] = np.array(MASK_SEED, dtype=np.int64)
        out["grad_streams"] = np.array(GRAD_STREAMS, dtype=np.int64)
        out["traj_streams"] = np.array(TRAJ_STREAMS, dtype=np.int64)
        for tag, extra in SETTINGS.items():
            cfg = G.base_config("IMPGCN", **common, **extra)
            groups = int(cfg["group"])
            ref_tools.set_seed(G.SEED)
            m = RefIMPGCN(cfg, data, G.CPU)
            small = [m.fc.weight, m.fc.bias, m.fc_group.weight, m.fc_group.bias]
            assert [id(p) for p in m.parameters()] == [id(m.user_embedding.weight), id(m.item_embedding.weight)] + [id(p) for p in small]
            if tag == "def":
                out["init_user"] = m.user_embedding.weight.detach().numpy().copy()
                out["init_item"] = m.item_embedding.weight.detach().numpy().copy()
                out["fc_weight"] = m.fc.weight.detach().numpy().copy()
                out["fc_bias"] = m.fc.bias.detach().numpy().copy()
            else:
                for key, t in (("init_user", m.user_embedding.weight), ("init_item", m.item_embedding.weight), ("fc_weight", m.fc.weight),
                               ("fc_bias", m.fc.bias)):
                    assert np.array_equal(out[key], t.detach().numpy())
            out[tag + "_fc_group_weight"] = m.fc_group.weight.detach().numpy().copy()
            out[tag + "_fc_group_bias"] = m.fc_group.bias.detach().numpy().copy()
            small0 = [p.detach().clone() for p in small]
            seen = record_membership(m)
            # ---- evaluation mode
            m.eval()
            with torch.no_grad():
                users, items = m.aggregate()
                out[tag + "_eval_member"] = member_bytes(seen, groups)
                out[tag + "_eval_user"] = users.numpy().copy()
                out[tag + "_eval_item"] = items.numpy().copy()
                out[tag + "_rating"] = m.get_rating_for_test(test_users).numpy()
            # ---- training mode, the published masks
            m.train()
            m.dropout = PublishedDropout(GRAD_STREAMS)
            m.zero_grad()
            ll = m(bu, bp, bn)
            sum(ll).backward()
            assert m.dropout.calls == 2
            out[tag + "_member"] = member_bytes(seen, groups)
            out[tag + "_loss"] = np.array([x.item() for x in ll])
            out[tag + "_grad_user"] = m.user_embedding.weight.grad.numpy().copy()
            out[tag + "_grad_item"] = m.item_embedding.weight.grad.numpy().copy()
            out[tag + "_fc_grad_is_none"] = np.array([p.grad is None for p in small])
            opt = torch.optim.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
            traj, members = [], []
            for i in range(3):
                b = tri3[i * 256:(i + 1) * 256]
                m.dropout = PublishedDropout(TRAJ_STREAMS[i])
                ll = m(b[:, 0], b[:, 1], b[:, 2])
                opt.zero_grad()
                sum(ll).backward()
                opt.step()
                traj.append([x.item() for x in ll])
                members.append(member_bytes(seen, groups))
            out[tag + "_traj_loss"] = np.array(traj)
            out[tag + "_traj_member"] = np.stack(members)
            out[tag + "_traj_user"] = m.user_embedding.weight.detach().numpy().copy()
            out[tag + "_traj_item"] = m.item_embedding.weight.detach().numpy().copy()
            out[tag + "_traj_fc_unchanged"] = np.array([torch.equal(p.detach(), p0) for p, p0 in zip(small, small0)])
        G.golden_io.save_npz(os.path.join(G.OUT, "impgcn_small.npz"), **out)
        print("wrote impgcn_small.npz (%d arrays)" % len(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
