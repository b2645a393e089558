"""ms per NCL training step and per E-step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, k = 2000
(configure/NCL.txt), one JSON line: the fused step before and after the warm-up (K products, fused BPR, two
idg_table_nce_f32 calls, after the warm-up idg_infonce_pair_f32 against the centroid panel, the backward chain, dense
Adam), the same model through forward() + autograd + ops.Adam, the reference's expressions as plain torch on the device
(torch.sparse.mm layers, two materialised [B, N] score matrices, the in-batch prototype term, torch.optim.Adam), and the
E-step — both tables, kmeans_niter iterations and the final assignment — through idg_kmeans_f32 and as plain torch
(mm, argmin, index_add_: it materialises [N, K]) from the same initial centroids.  Device events after a warm-up; the step
figures are the median of --windows windows of --steps steps, the E-step figures the median of --windows runs.
--fused-only times the fused step after the warm-up and the E-step and nothing else (what a kernel trace is taken from:
profiles/ncl/).

    python scripts/ncl_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch] [--fused-only]
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


def torch_kmeans(X, first, niter):
    """Lloyd's iterations as plain torch from the rows `first` (an empty cluster keeps its centroid), then the assignment."""
    C = X[first].clone()
    xn = (X * X).sum(dim=1)

    def nearest():
        return (xn[:, None] - 2.0 * torch.mm(X, C.t()) + (C * C).sum(dim=1)[None, :]).argmin(dim=1)

    for _ in range(niter):
        a = nearest()
        cnt = torch.bincount(a, minlength=C.shape[0])
        s = torch.zeros_like(C).index_add_(0, a, X)
        C = torch.where(cnt[:, None] > 0, s / cnt.clamp_min(1)[:, None], C)
    return C, nearest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch compositions")
    ap.add_argument("--fused-only", action="store_true", help="time the fused step after the warm-up and the E-step only")
    args = ap.parse_args()
    from models.NCL import NCL

    root = tempfile.mkdtemp(prefix="idg_ncl_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "NCL.txt"), "NCL")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K = 2048, 64, data.num_users, data.num_items, int(cfg["GCN_layer"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    tm = lambda step, div=1: _time(step, batches, max(2, args.steps // div), max(1, args.warmup // div), args.windows)  # noqa: E731

    tools.set_seed(2024)
    m = NCL(cfg, data, torch.device("cuda")).to("cuda")
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "k": m.k, "kmeans_niter": m.kmeans_niter,
           "steps": args.steps, "windows": args.windows}
    opt = ops.Adam(m.parameters(), lr=0.001)
    loss = torch.zeros(4, device="cuda")
    m.train()

    def e_step_ms(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1))
        return statistics.median(ts)

    out["e_step_ms"] = e_step_ms(m.E_step)
    flop = 2.0 * (U + I) * m.k * d * (m.kmeans_niter + 1)
    out["e_step_assign_tflops_lower_bound"] = flop / (out["e_step_ms"] * 1e-3) / 1e12  # the whole E-step's time under the assigns' flops
    m.epoch = m.proto_warmup
    out["fused_after_warmup_ms"] = tm(lambda b: m.fused_train_step(*b, loss, opt))
    if args.fused_only:
        print(json.dumps(out))
        return
    m.epoch = 0
    out["fused_before_warmup_ms"] = tm(lambda b: m.fused_train_step(*b, loss, opt))

    def autograd_step(b):
        ll = m(*b)
        opt.zero_grad()
        sum(ll).backward()
        opt.step()

    out["autograd_before_warmup_ms"] = tm(autograd_step)
    m.epoch = m.proto_warmup
    out["autograd_after_warmup_ms"] = tm(autograd_step)

    if not args.skip_torch:
        st = m._storage
        firsts = [torch.randperm(n, generator=torch.Generator().manual_seed(m.kmeans_seed))[:m.k].cuda() for n in (U, I)]

        def torch_e_step():
            return torch_kmeans(st[:U], firsts[0], m.kmeans_niter), torch_kmeans(st[U:], firsts[1], m.kmeans_niter)

        out["torch_e_step_ms"] = e_step_ms(torch_e_step)
        out["e_step_over_torch"] = out["e_step_ms"] / out["torch_e_step_ms"]
        # the two E-steps start from the same rows: how many rows end in the same cluster (fp32 orders differ, so near-ties
        # may part ways and the runs drift apart from there)
        m.E_step()
        (_, tu), (_, ti) = torch_e_step()
        out["e_step_rows_agreeing_with_torch"] = float(((tu == m.user_2cluster).sum() + (ti == m.item_2cluster).sum()).item()) / (U + I)

        # the reference's expressions (models/NCL.py:48-142) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        torch.nn.init.xavier_uniform_(ue.weight, gain=1)
        torch.nn.init.xavier_uniform_(ie.weight, gain=1)
        topt = torch.optim.Adam(list(ue.parameters()) + list(ie.parameters()), lr=0.001)
        F = torch.nn.functional
        tau, L = m.temperature, 2 * m.cl_layer
        uc, u2c, ic, i2c = m.user_centroids, m.user_2cluster, m.item_centroids, m.item_2cluster

        def side(query, table, positive):
            q, t = F.normalize(query), F.normalize(table)
            pos = torch.exp((q * t[positive]).sum(dim=1) / tau)
            ttl = torch.exp(torch.matmul(q, t.transpose(0, 1)) / tau).sum(dim=1)
            return -torch.log(pos / ttl + 10e-8).sum()

        def torch_step(b, proto):
            users, pos, neg = b
            x = torch.cat([ue.weight, ie.weight])
            layers = [x]
            for _ in range(K):
                x = torch.sparse.mm(A, x)
                layers.append(x)
            fu, fi = torch.split(torch.stack(layers, dim=1).mean(dim=1), [U, I])
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg])
            total = total + m.reg_lambda * losses.get_reg_loss(ue(users), ie(pos), ie(neg))
            eu, ei = torch.split(layers[0], [U, I])
            lu, li = torch.split(layers[L], [U, I])
            total = total + m.ssl_lambda * (side(lu[users], eu, users) + m.alpha * side(li[pos], ei, pos))
            if proto:
                total = total + m.proto_lambda * B * (losses.get_InfoNCE_loss(eu[users], uc[u2c[users]], tau)
                                                      + losses.get_InfoNCE_loss(ei[pos], ic[i2c[pos]], tau))
            topt.zero_grad()
            total.backward()
            topt.step()

        out["torch_before_warmup_ms"] = tm(lambda b: torch_step(b, False), 2)
        out["torch_after_warmup_ms"] = tm(lambda b: torch_step(b, True), 2)
        out["fused_over_torch_after_warmup"] = out["fused_after_warmup_ms"] / out["torch_after_warmup_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
