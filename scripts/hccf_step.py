"""ms per HCCF training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = hyper_size = 64, B = 2048, K = 3
(configure/HCCF.txt), one JSON line: the fused step (idgrec_amd/hccf.py), the same model through forward() + autograd +
ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm, dense matmuls, F.dropout,
get_InfoNCE_loss, torch.optim.Adam), and the fused LightGCN step at the same shape — the yardstick of what the propagation
and BPR alone cost.  Every timed shape is warmed first; then the four are ALTERNATED: window w times --steps steps of each in
turn, and every figure is the median of the --windows windows, with the windows' min and max next to it.

Each of the four hypergraph kernels alone, on panels of the step's size (all n rows as one side, generated masks at
keep = 0.5 so that the mask's arithmetic is in the figure): ms, effective GB/s over the panels it reads and writes (latent:
E0 and X; expand with side / next / total: E0, side, total in, Y, next, total out; backward with accumulate: E0, X, gY, gX, gHb in, gX and gHb out;
close: E0, gHb, gE0 in, gE0 out) and TFLOP/s over 2 n d h per product (latent 2, expand 2, backward 4, close 2 — the
recomputed E0 . W counts).  The panels (18 MB each) live in the Infinity Cache, so the GB/s are not a share of the HBM peak.

    python scripts/hccf_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    args = ap.parse_args()
    from models.HCCF import HCCF
    from models.LightGCN import LightGCN

    root = tempfile.mkdtemp(prefix="idg_hccf_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "HCCF.txt"), "HCCF")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", hyper_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, h, U, I, K = 2048, 64, 64, data.num_users, data.num_items, int(cfg["GCN_layer"])
    n = U + I
    reg, lam, t, keep = float(cfg["reg_lambda"]), float(cfg["ssl_lambda"]), float(cfg["temperature"]), float(cfg["keeprate"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "h": h, "B": B, "U": U, "I": I, "layers": K, "keeprate": keep, "steps": args.steps,
           "windows": args.windows}
    loss = torch.zeros(3, device="cuda")

    tools.set_seed(2024)
    m = HCCF(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    m.train()
    assert m.fused_step_available()

    # the same model once more for the autograd path: the fused step keeps the hyperedge matrices in the engine's flat buffer
    tools.set_seed(2024)
    ma = HCCF(cfg, data, torch.device("cuda")).to("cuda")
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
    lcfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048", GCN_layer=str(K))
    tools.set_seed(2024)
    lg = LightGCN(lcfg, data, torch.device("cuda")).to("cuda")
    lopt = ops.Adam(lg.parameters(), lr=float(lcfg["learn_rate"]))
    lg.train()
    assert lg.fused_step_available()

    def lightgcn_step(b):
        assert lg.fused_train_step(*b, loss[:2], lopt)

    named = [("fused", fused_step), ("autograd", autograd_step), ("lightgcn_fused", lightgcn_step)]
    if not args.skip_torch:
        # the reference's expressions (models/HCCF.py:49-119) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        uh, ih = torch.nn.Embedding(d, h).cuda(), torch.nn.Embedding(d, h).cuda()
        for e in (ue, ie, uh, ih):
            torch.nn.init.xavier_uniform_(e.weight, gain=1.)
        topt = torch.optim.Adam([e.weight for e in (ue, ie, uh, ih)], lr=float(cfg["learn_rate"]))

        def torch_step(b):
            users, pos, neg = b
            embs = [torch.cat([ue.weight, ie.weight])]
            gnn, hyp = [], []
            uu, ii = ue.weight @ uh.weight, ie.weight @ ih.weight
            for _ in range(K):
                s = torch.sparse.mm(A, embs[-1])
                hu, hi = torch.nn.functional.dropout(uu, p=1 - keep), torch.nn.functional.dropout(ii, p=1 - keep)
                y = torch.cat([hu @ (hu.T @ embs[-1][:U]), hi @ (hi.T @ embs[-1][U:])])
                gnn.append(s)
                hyp.append(y)
                embs.append(s + y)
            final = sum(embs)
            fu, fi = final[:U], final[U:]
            ssl = 0.
            for s, y in zip(gnn, hyp):
                s = s.detach()
                ssl = ssl + losses.get_InfoNCE_loss(s[:U][users], y[:U][users], t) + losses.get_InfoNCE_loss(s[U:][pos], y[U:][pos], t)
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg]) \
                + reg * losses.get_reg_loss(ue(users), ie(pos), ie(neg), uh.weight, ih.weight) + lam * ssl
            topt.zero_grad()
            total.backward()
            topt.step()

        named.append(("torch", torch_step))

    for name, (med, lo, hi) in _alternate(named, batches, args.steps, args.warmup, args.windows).items():
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
    out["fused_over_lightgcn_fused"] = out["fused_ms"] / out["lightgcn_fused_ms"]
    out["fused_over_autograd"] = out["fused_ms"] / out["autograd_ms"]
    if not args.skip_torch:
        out["fused_over_torch"] = out["fused_ms"] / out["torch_ms"]

    # the four hypergraph kernels alone, on panels of the step's size
    gen = torch.Generator(device="cuda").manual_seed(1)
    E0, X, gY, side = (torch.randn(n, d, device="cuda", generator=gen) * 0.1 for _ in range(4))
    W = torch.randn(d, h, device="cuda", generator=gen) * 0.1
    L, gL, gW = (torch.empty(h, d, device="cuda") for _ in range(3))
    Y, nxt, total, gX, gE0 = (torch.zeros(n, d, device="cuda") for _ in range(5))
    gHb = torch.empty(n, h, device="cuda")
    kw = dict(keep=0.5, seed=1234, stream_id=7)
    ops.hyper_latent_raw(E0, W, X, L, **kw)
    ops.hyper_latent_raw(E0, W, gY, gL, **kw)
    panel, flop = n * d * 4, 2.0 * n * d * h
    alone = _alternate([("hyper_latent", lambda _: ops.hyper_latent_raw(E0, W, X, L, **kw)),
                        ("hyper_expand", lambda _: ops.hyper_expand_raw(E0, W, L, Y, side=side, next=nxt, total=total, **kw)),
                        ("hyper_bwd", lambda _: ops.hyper_bwd_raw(E0, W, X, gY, L, gL, gX, gHb, accumulate=True, **kw)),
                        ("hyper_close", lambda _: ops.hyper_close_raw(E0, W, gHb, gE0, gW))],
                       batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    for name, panels, products in (("hyper_latent", 2, 2), ("hyper_expand", 6, 2), ("hyper_bwd", 7, 4), ("hyper_close", 4, 2)):
        med, lo, hi = alone[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        out[name + "_gbs"] = panels * panel / (med * 1e-3) / 1e9
        out[name + "_tflops"] = products * flop / (med * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
