"""ms per CGCL training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048 (configure/CGCL.txt's batch
size), one JSON line: the fused step (K products, fused BPR, four idg_table_nce_f32 calls, the backward chain, dense Adam),
the same model through forward() + autograd + ops.Adam, the reference's expressions as plain torch on the device
(torch.sparse.mm layers, six materialised [B, N] score matrices, torch.optim.Adam — the baseline the fused step is held
against), the fused LightGCN step at the same B, and the four table calls alone with their TFLOP/s counted as
4 x 2 B N d per query block.  Device events after a warm-up; every figure is the median of --windows windows of --steps
steps.  --fused-only times the fused step and nothing else (what a kernel trace is taken from: profiles/cgcl/).

    python scripts/cgcl_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch] [--fused-only]
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


def _time(step, batches, steps, warmup, windows):
    for i in range(warmup):
        step(batches[i % len(batches)])
    torch.cuda.synchronize()
    out = []
    for w in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(steps):
            step(batches[(w * steps + i) % len(batches)])
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / steps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    ap.add_argument("--fused-only", action="store_true", help="time the fused step only")
    args = ap.parse_args()
    from models.CGCL import CGCL
    from models.LightGCN import LightGCN

    root = tempfile.mkdtemp(prefix="idg_cgcl_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "CGCL.txt"), "CGCL")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K = 2048, 64, data.num_users, data.num_items, int(cfg["GCN_layer"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "steps": args.steps, "windows": args.windows}
    tm = lambda step, div=1: _time(step, batches, max(2, args.steps // div), max(1, args.warmup // div), args.windows)  # noqa: E731

    tools.set_seed(2024)
    m = CGCL(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=0.001)
    loss = torch.zeros(5, device="cuda")
    m.train()
    out["fused_ms"] = tm(lambda b: m.fused_train_step(*b, loss, opt))
    if args.fused_only:
        print(json.dumps(out))
        return

    def autograd_step(b):
        ll = m(*b)
        opt.zero_grad()
        sum(ll).backward()
        opt.step()

    out["autograd_ms"] = tm(autograd_step)

    # the four table calls alone, on the layers of the current weights
    with torch.no_grad():
        E = [x.contiguous() for x in m.aggregate()[2]]
    G = [torch.zeros_like(E[0]) for _ in range(3)]
    part = torch.zeros(2, device="cuda")

    def table_calls(b):
        users, pos = b[0], b[1]
        rows = pos + U
        for tl, row0, N, blocks, user_side in m._terms():
            ops.table_nce_raw(E[tl], row0, N, [E[ql] for ql, _, _ in blocks], [rows if user_side else users] * len(blocks),
                              users if user_side else pos, [w for _, w, _ in blocks], m.temperature, loss=part[:len(blocks)],
                              g_table=G[tl], g_queries=[G[ql] for ql, _, _ in blocks])

    out["table_calls_ms"] = tm(table_calls)
    flop = sum(len(blocks) * 4 * 2 * B * N * d for _, _, N, blocks, _ in m._terms())
    out["table_calls_tflops"] = flop / (out["table_calls_ms"] * 1e-3) / 1e12
    out["table_calls_share_of_fp32_matrix_peak"] = out["table_calls_tflops"] / 157.3

    tools.set_seed(2024)
    lcfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    lcfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    lg = LightGCN(lcfg, data, torch.device("cuda")).to("cuda")
    lopt = ops.Adam(lg.parameters(), lr=0.001)
    lloss = torch.zeros(2, device="cuda")
    out["lightgcn_fused_ms"] = tm(lambda b: lg.fused_train_step(*b, lloss, lopt))

    if not args.skip_torch:
        # the reference's expressions (models/CGCL.py:44-215) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        torch.nn.init.xavier_uniform_(ue.weight, gain=1)
        torch.nn.init.xavier_uniform_(ie.weight, gain=1)
        topt = torch.optim.Adam(list(ue.parameters()) + list(ie.parameters()), lr=0.001)
        F = torch.nn.functional
        tau = m.temperature

        def side(query, table, positive):
            q, t = F.normalize(query), F.normalize(table)
            pos = torch.exp((q * t[positive]).sum(dim=1) / tau)
            ttl = torch.exp(torch.matmul(q, t.transpose(0, 1)) / tau).sum(dim=1)
            return -torch.log(pos / ttl + 10e-8).sum()

        def pair(later, earlier, users, pos, lam, mix):
            lu, li = torch.split(later, [U, I])
            eu, ei = torch.split(earlier, [U, I])
            return lam * (mix * side(li[pos], eu, users) + (1 - mix) * side(lu[users], ei, pos))

        def torch_step(b):
            users, pos, neg = b
            x = torch.cat([ue.weight, ie.weight])
            layers = [x]
            for _ in range(K):
                x = torch.sparse.mm(A, x)
                layers.append(x)
            fu, fi = torch.split(torch.stack(layers, dim=1).mean(dim=1), [U, I])
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg])
            total = total + m.reg_lambda * losses.get_reg_loss(ue(users), ie(pos), ie(neg))
            total = total + pair(layers[2], layers[0], users, pos, m.ssl_lambda_alpha, m.alpha)
            total = total + pair(layers[1], layers[0], users, pos, m.ssl_lambda_beta, m.beta)
            total = total + pair(layers[2], layers[1], users, pos, m.ssl_lambda_gamma, m.gamma)
            topt.zero_grad()
            total.backward()
            topt.step()

        out["torch_ms"] = tm(torch_step, 2)
        out["fused_over_torch"] = out["fused_ms"] / out["torch_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
