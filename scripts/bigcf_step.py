"""ms per BIGCF training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, intent_size = 128, B = 2048, K = 2
(configure/BIGCF.txt), one JSON line: the fused step (idgrec_amd/bigcf.py), the same model through forward() + autograd +
ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm, torch.softmax, torch.randn_like,
get_InfoNCE_loss, torch.optim.Adam), and the fused LightGCN step at the same shape — the yardstick of what the propagation
and BPR alone cost.  Every timed shape is warmed first; then the four are ALTERNATED: window w times --steps steps of each in
turn, and every figure is the median of the --windows windows, with the windows' min and max next to it.

Each of the two intent kernels alone, on panels of the step's size and all rows (the backward also at one batch's bitmap, as the
step calls it): ms, effective GB/s over its minimal traffic (forward: read X, write T and F; backward: read X, gF and gT, write
gX) and TFLOP/s over 2 n d k per product (forward: two products; backward: five).  The panels (18 MB each) live in the
Infinity Cache, so the GB/s are not a share of the HBM peak.

    python scripts/bigcf_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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
    from models.BIGCF import BIGCF
    from models.LightGCN import LightGCN

    root = tempfile.mkdtemp(prefix="idg_bigcf_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "BIGCF.txt"), "BIGCF")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", intent_size="128", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, k, U, I, K = 2048, 64, 128, data.num_users, data.num_items, int(cfg["GCN_layer"])
    n = U + I
    reg, lam, t = float(cfg["reg_lambda"]), float(cfg["ssl_lambda"]), float(cfg["ssl_temperature"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "k": k, "B": B, "U": U, "I": I, "layers": K, "steps": args.steps, "windows": args.windows}
    loss = torch.zeros(3, device="cuda")

    tools.set_seed(2024)
    m = BIGCF(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    m.train()
    assert m.fused_step_available()

    # the same model once more for the autograd path: the fused step keeps the intent matrices in the engine's flat buffer
    tools.set_seed(2024)
    ma = BIGCF(cfg, data, torch.device("cuda")).to("cuda")
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
        # the reference's expressions (models/BIGCF.py:46-106) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        ui, ii = torch.nn.Embedding(d, k).cuda(), torch.nn.Embedding(d, k).cuda()
        for e in (ue, ie, ui, ii):
            torch.nn.init.xavier_uniform_(e.weight, gain=1.)
        topt = torch.optim.Adam([e.weight for e in (ue, ie, ui, ii)], lr=float(cfg["learn_rate"]))

        def torch_step(b):
            users, pos, neg = b
            x = torch.cat([ue.weight, ie.weight])
            layers = []
            for _ in range(K):
                x = torch.sparse.mm(A, x)
                layers.append(x)
            gnn = torch.sum(torch.stack(layers, dim=1), dim=1)
            gu, gi = torch.split(gnn, [U, I])
            intent = torch.cat([torch.softmax(gu @ ui.weight, dim=1) @ ui.weight.T, torch.softmax(gi @ ii.weight, dim=1) @ ii.weight.T])
            final = gnn + intent * torch.randn_like(gnn)
            fu, fi = torch.split(final, [U, I])
            tu, ti = torch.split(intent, [U, I])
            u, p, q = fu[users], fi[pos], fi[neg]
            ssl = losses.get_InfoNCE_loss(u, u, t) + losses.get_InfoNCE_loss(p, p, t) + losses.get_InfoNCE_loss(u, p, t) \
                + losses.get_InfoNCE_loss(tu[users], tu[users], t) + losses.get_InfoNCE_loss(ti[pos], ti[pos], t)
            total = losses.get_bpr_loss(u, p, q) + reg * losses.get_reg_loss(ue(users), ie(pos), ie(neg), ui.weight, ii.weight) + lam * ssl
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

    # the two intent kernels alone, on panels of the step's size
    gen = torch.Generator(device="cuda").manual_seed(1)
    X, gF, gT = (torch.randn(n, d, device="cuda", generator=gen) for _ in range(3))
    W = torch.randn(d, k, device="cuda", generator=gen) * 0.1
    T, F, gX, gW = torch.empty_like(X), torch.empty_like(X), torch.zeros_like(X), torch.empty(d, k, device="cuda")
    bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    ops.bpr_touch_rows_raw(*batches[0], U, bitmap, clear_bits=n)
    out["batch_rows"] = int(sum(bin(w & 0xFFFFFFFF).count("1") for w in bitmap.cpu().tolist()))
    panel, flop = n * d * 4, 2.0 * n * d * k
    alone = _alternate([("intent_fwd", lambda _: ops.intent_fwd_raw(X, W, T, F, seed=1234, stream_id=7)),
                        ("intent_bwd", lambda _: ops.intent_bwd_raw(gF, gT, None, X, W, gX, gW, seed=1234, stream_id=7)),
                        ("intent_bwd_batch_rows", lambda _: ops.intent_bwd_raw(gF, gT, bitmap, X, W, gX, gW, seed=1234, stream_id=7))],
                       batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    for name, traffic, products in (("intent_fwd", 3 * panel, 2), ("intent_bwd", 4 * panel, 5), ("intent_bwd_batch_rows", None, None)):
        med, lo, hi = alone[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        if traffic is not None:
            out[name + "_gbs"] = traffic / (med * 1e-3) / 1e9
            out[name + "_tflops"] = products * flop / (med * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
