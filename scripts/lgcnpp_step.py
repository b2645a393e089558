"""ms per LightGCN++ training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048
(configure/LightGCN_pp.txt), one JSON line: the fused step (K x (rows_normalize + product), fused BPR, K x (transposed
product + rows_normalize_bwd), dense Adam), the same model through forward() + autograd + ops.Adam, the reference's
expressions as plain torch on the device (torch.norm, the division, torch.sparse.mm, torch.optim.Adam), the fused LightGCN
step at the same shape, and each of the two row-normalisation kernels alone with its effective GB/s over its minimal traffic
(forward: one panel read, one written, plus the norms; backward: T, Y, G read, out written, plus the norms).  Device events
after a warm-up; every figure is the median of --windows windows of --steps steps.  The panels (18 MB each) live in the
Infinity Cache, so the GB/s are not a share of the HBM peak.

    python scripts/lgcnpp_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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
    args = ap.parse_args()
    from models.LightGCN import LightGCN
    from models.LightGCN_pp import LightGCN_pp

    root = tempfile.mkdtemp(prefix="idg_lgcnpp_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN_pp.txt"), "LightGCN_pp")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K = 2048, 64, data.num_users, data.num_items, int(cfg["GCN_layer"])
    n = U + I
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    tm = lambda step, div=1: _time(step, batches, max(2, args.steps // div), max(1, args.warmup // div), args.windows)  # noqa: E731

    tools.set_seed(2024)
    m = LightGCN_pp(cfg, data, torch.device("cuda")).to("cuda")
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "alpha": m.alpha, "beta": m.beta, "gamma": m.gamma,
           "steps": args.steps, "windows": args.windows}
    opt = ops.Adam(m.parameters(), lr=0.001)
    loss = torch.zeros(2, device="cuda")
    m.train()
    out["fused_ms"] = tm(lambda b: m.fused_train_step(*b, loss, opt))

    def autograd_step(b):
        ll = m(*b)
        opt.zero_grad()
        sum(ll).backward()
        opt.step()

    out["autograd_ms"] = tm(autograd_step)
    out["fused_over_autograd"] = out["fused_ms"] / out["autograd_ms"]

    # the two row kernels alone, on panels of the step's size
    gen = torch.Generator(device="cuda").manual_seed(1)
    X, T, G = (torch.randn(n, d, device="cuda", generator=gen) for _ in range(3))
    Y, norms, res = torch.empty_like(X), torch.empty(n, device="cuda"), torch.empty_like(X)
    panel = n * d * 4
    ms = tm(lambda b: ops.rows_normalize_raw(X, Y=Y, norms=norms), 1)
    out["rows_normalize_ms"], out["rows_normalize_gbs"] = ms, (2 * panel + n * 4) / (ms * 1e-3) / 1e9
    ms = tm(lambda b: ops.rows_normalize_bwd_raw(T, Y, norms, G=G, a=0.2, out=res), 1)
    out["rows_normalize_bwd_ms"], out["rows_normalize_bwd_gbs"] = ms, (4 * panel + n * 4) / (ms * 1e-3) / 1e9

    # the fused LightGCN step at the same shape
    lcfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCN.txt"), "LightGCN")
    lcfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048",
                GCN_layer=str(K))
    tools.set_seed(2024)
    lg = LightGCN(lcfg, data, torch.device("cuda")).to("cuda")
    lopt = ops.Adam(lg.parameters(), lr=0.001)
    lg.train()
    out["lightgcn_fused_ms"] = tm(lambda b: lg.fused_train_step(*b, loss, lopt))
    out["fused_over_lightgcn_fused"] = out["fused_ms"] / out["lightgcn_fused_ms"]

    if not args.skip_torch:
        # the reference's expressions (models/LightGCN_pp.py:75-116) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix_asymmetric(data, m.alpha, m.beta)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        torch.nn.init.xavier_uniform_(ue.weight, gain=1)
        torch.nn.init.xavier_uniform_(ie.weight, gain=1)
        topt = torch.optim.Adam(list(ue.parameters()) + list(ie.parameters()), lr=0.001)

        def torch_step(b):
            users, pos, neg = b
            x = e0 = torch.cat([ue.weight, ie.weight])
            layers = []
            for _ in range(K):
                x = x / (torch.norm(x, dim=1) + 1e-12)[:, None]
                x = torch.sparse.mm(A, x)
                layers.append(x)
            final = m.gamma * e0 + (1 - m.gamma) * torch.mean(torch.stack(layers, dim=1), dim=1)
            fu, fi = torch.split(final, [U, I])
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg])
            total = total + m.reg_lambda * losses.get_reg_loss(ue(users), ie(pos), ie(neg))
            topt.zero_grad()
            total.backward()
            topt.step()

        out["torch_ms"] = tm(torch_step, 2)
        out["fused_over_torch"] = out["fused_ms"] / out["torch_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
