"""ms per IMP-GCN training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, group = 3, GCN_layer = 6
(configure/IMPGCN.txt), one JSON line: the fused step (idgrec_amd/impgcn.py), the same model through forward() + autograd +
ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm over freshly built sub-graph tensors,
nn.Linear, nn.LeakyReLU, nn.Dropout, torch.topk / torch.eq, torch.optim.Adam), and the fused LightGCN step — the yardstick:
LightGCN runs 3 plain products per direction where IMP-GCN runs 1 plain + 5 grouped ones.  Every timed shape is warmed first;
then the four are ALTERNATED: window w times --steps steps of each in turn, and every figure is the median of the --windows
windows, with the windows' min and max next to it.

Each kernel alone, on panels of the step's size: ms and effective GB/s over its minimal traffic.  The assignment: read ego
and side, write one byte per node.  The grouped product (a middle product of the chain: grouped X, Y and S with S_in): per
entry 9 bytes of index, value and membership, 256 bytes per gather — one for every group the entry's two endpoints share —
and the rows written; with the evaluation-mode membership (one group per user) and with a training-mode one (ties from
Dropout(0.4)), each next to THE SAME RESULT COMPOSED FROM WHAT EXISTED BEFORE: per group the rows masked in torch, the
library's tuned product (Graph.spmm_raw), masked again, and the sum — alternated in the same way.  The panels live in the
Infinity Cache, so the GB/s are not a share of the HBM peak.

    python scripts/impgcn_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import idgrec_amd.synth as S  # noqa: E402
import utility.utility_data.data_graph as data_graph  # noqa: E402
import utility.utility_data.data_loader as data_loader  # noqa: E402
import utility.utility_function.losses as losses  # noqa: E402
import utility.utility_function.tools as tools  # noqa: E402
from idgrec_amd import ops  # noqa: E402


def _window(step, batches, steps, w):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        step(batches[(w * steps + i) % len(batches)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def _alternate(named, batches, steps, warmup, windows):
    """{name: (median, min, max)} of `windows` windows per step function, the functions taking turns inside every window."""
    for _, step in named:
        for i in range(warmup):
            step(batches[i % len(batches)])
    torch.cuda.synchronize()
    seen = {name: [] for name, _ in named}
    for w in range(windows):
        for name, step in named:
            seen[name].append(_window(step, batches, steps, w))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in seen.items()}


def _steps(args, root, data, batches, cfg):
    """The four step contenders."""
    from models.IMPGCN import IMPGCN
    from models.LightGCN import LightGCN

    d, U, I = 64, data.num_users, data.num_items
    G, L = int(cfg["group"]), int(cfg["GCN_layer"])
    loss = torch.zeros(2, device="cuda")
    tools.set_seed(2024)
    m = IMPGCN(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    m.train()
    assert m.fused_step_available()
    # the same model once more for the autograd path: the fused step keeps its small tensors in the engine's flat buffer
    tools.set_seed(2024)
    ma = IMPGCN(cfg, data, torch.device("cuda")).to("cuda")
    aopt = ops.Adam(ma.parameters(), lr=float(cfg["learn_rate"]))
    ma.train()

    def fused_step(b):
        assert m.fused_train_step(*b, loss, opt)

    def autograd_step(b):
        ll = ma(*b)
        aopt.zero_grad()
        sum(ll).backward()
        aopt.step()

    lcfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    lcfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    tools.set_seed(2024)
    lg = LightGCN(lcfg, data, torch.device("cuda")).to("cuda")
    lopt = ops.Adam(lg.parameters(), lr=float(lcfg["learn_rate"]))
    lg.train()
    assert lg.fused_step_available()

    def lightgcn_step(b):
        assert lg.fused_train_step(*b, loss, lopt)

    named = [("fused", fused_step), ("autograd", autograd_step), ("lightgcn_fused", lightgcn_step)]
    if not args.skip_torch:
        # the reference's expressions (models/IMPGCN.py:50-108) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        torch.nn.init.xavier_uniform_(ue.weight, gain=1)
        torch.nn.init.xavier_uniform_(ie.weight, gain=1)
        fc, fc_group = torch.nn.Linear(d, d).cuda(), torch.nn.Linear(d, G).cuda()
        leaky, drop = torch.nn.LeakyReLU(), torch.nn.Dropout(p=0.4)
        topt = torch.optim.Adam(list(ue.parameters()) + list(ie.parameters()) + list(fc.parameters()) + list(fc_group.parameters()),
                                lr=float(cfg["learn_rate"]))

        def subgraph(graph, group, dim):
            index, value = graph._indices(), graph._values()
            return torch.sparse_coo_tensor(index, value * group[index[dim, :]], graph.size())

        def torch_step(b):
            users, pos, neg = b
            ego = torch.cat([ue.weight, ie.weight])
            temp = drop(leaky(fc(ego + torch.sparse.mm(A, ego))))
            scores = drop(fc_group(temp))
            top, _ = torch.topk(scores, k=1, sorted=False)
            hot = torch.eq(scores, top).float()
            hot = torch.cat([hot[:U], torch.ones((I, G), device="cuda")]).t()
            graphs = [subgraph(subgraph(A, hot[g], 1), hot[g], 0) for g in range(G)]
            layers = [[ego] * G]
            for _ in range(1, L):
                layers.append([torch.sparse.mm(graphs[g], layers[-1][g]) for g in range(G)])
            final = torch.mean(torch.stack([torch.sum(torch.stack(x), 0) for x in layers], dim=1), dim=1)
            fu, fi = torch.split(final, [U, I])
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg]) + m.reg_lambda * losses.get_reg_loss(ue(users), ie(pos), ie(neg))
            topt.zero_grad()
            total.backward()
            topt.step()

        named.append(("torch", torch_step))
    res = {}
    for name, (med, lo, hi) in _alternate(named, batches, args.steps, args.warmup, args.windows).items():
        res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = med, lo, hi
    res["fused_over_lightgcn_fused"] = res["fused_ms"] / res["lightgcn_fused_ms"]
    res["fused_over_autograd"] = res["fused_ms"] / res["autograd_ms"]
    if not args.skip_torch:
        res["fused_over_torch"] = res["fused_ms"] / res["torch_ms"]
    return res, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    args = ap.parse_args()

    root = tempfile.mkdtemp(prefix="idg_impgcn_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "IMPGCN.txt"), "IMPGCN")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I = 2048, 64, data.num_users, data.num_items
    n, G, L = U + I, int(cfg["group"]), int(cfg["GCN_layer"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "group": G, "GCN_layer": L, "steps": args.steps,
           "windows": args.windows}
    step, m = _steps(args, root, data, batches, cfg)
    out.update(step)

    # the kernels alone, on panels of the step's size and the model's own graph and weights
    csr, graph = m.group_csr(), m.Graph
    out["nnz"], out["long_rows"], out["long_row_chunks"] = csr.nnz, csr.n_long, csr.n_chunks
    gen = torch.Generator(device="cuda").manual_seed(1)
    ego = m._storage
    side = graph.spmm_raw(ego)
    small = (m.fc.weight.data, m.fc.bias.data, m.fc_group.weight.data, m.fc_group.bias.data)
    member = {"eval": ops.group_assign_raw(ego, side, *small, U, 0.0, 0, 0, 0).clone(),
              "train": ops.group_assign_raw(ego, side, *small, U, 0.4, 1234, 1, 2).clone()}
    X, V, S_in = torch.randn(G, n, d, device="cuda", generator=gen), None, torch.randn(n, d, device="cuda", generator=gen)
    Y, Ssum, scratch = torch.empty_like(X), torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
    panel = n * d * 4
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), csr.indptr[1:] - csr.indptr[:-1])
    scratch_member = torch.empty(n, dtype=torch.uint8, device="cuda")
    named = [("assign", lambda _: ops.group_assign_raw(ego, side, *small, U, 0.4, 1234, 1, 2, member=scratch_member))]
    traffic = {"assign": 2 * panel + n}
    for mode, mem in member.items():
        hot = [((mem >> g) & 1).to(torch.float32)[:, None] for g in range(G)]
        shared = (mem[rows] & mem[csr.indices.long()]).to(torch.int32)
        gathers = int(sum(((shared >> g) & 1).sum() for g in range(G)))
        written = int(sum(h.sum() for h in hot))
        out["multi_group_users_" + mode] = float(((mem[:U] & (mem[:U] - 1)) != 0).float().mean())
        out["gathers_per_entry_" + mode] = gathers / csr.nnz
        traffic["grouped_" + mode] = 9 * csr.nnz + 256 * gathers + 256 * written + 2 * panel

        def grouped(_, mem=mem):
            ops.grouped_spmm_raw(csr, mem, X, G, V=V, Y=Y, S=Ssum, S_in=S_in)

        def composed(_, hot=hot):
            total = S_in
            for g in range(G):
                graph.spmm_raw(X[g] * hot[g], out=scratch)
                torch.mul(scratch, hot[g], out=Y[g])
                total = total + Y[g]
            return total

        named += [("grouped_" + mode, grouped), ("composed_" + mode, composed)]
    alone = _alternate(named, batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    for name, (med, lo, hi) in alone.items():
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        if name in traffic:
            out[name + "_gbs"] = traffic[name] / (med * 1e-3) / 1e9
    for mode in member:
        out["grouped_over_composed_" + mode] = out["grouped_%s_ms" % mode] / out["composed_%s_ms" % mode]
    out["plain_spmm_ms"] = _alternate([("plain", lambda _: graph.spmm_raw(ego, out=scratch))], batches, 50, 10, args.windows)["plain"][0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
