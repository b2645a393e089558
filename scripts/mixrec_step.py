"""ms per MixRec training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, GCN_layer = 3
(configure/MixRec.txt), one JSON line: the fused step (idgrec_amd/mixrec.py), the same model through forward() + autograd +
ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm, get_InfoNCE_loss_all four times per
side pair plus once for the mixed negatives, torch.optim.Adam), and the fused LightGCN step at the same shape — the yardstick
of what the propagation and BPR alone cost.  Every timed shape is warmed first; then the four are ALTERNATED: window w times
--steps steps of each in turn, and every figure is the median of the --windows windows, with the windows' min and max next to
it.  All four draw their Beta / Dirichlet / permutation numbers on the host every step, as the reference does.

idg_mix_nce_f32 alone on a panel of the step's size, forward (losses only) and forward + backward, against the same five
terms in plain torch on the gathered rows (forward, and forward + backward through autograd): ms, and TFLOP/s over the
matrix products the kernel actually performs on its zero-padded operands — 2 Bp^2 dp per product, Bp = B rounded up to 128,
dp = d rounded up to 32; three problems; the loss-only call forms each score tile once (3 products), the gradient call forms
it twice and multiplies it into the rows twice (12 products).

    python scripts/mixrec_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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
from idgrec_amd.mixrec import draw_mix  # noqa: E402


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


def torch_terms(u, p, q, draws, t, lam):
    """The reference's five contrastive calls (models/MixRec.py:100-150) on gathered rows, plain torch."""
    user_beta, item_beta, nu, user_index, item_index = draws
    neg_beta = nu.reshape(1, -1, 1)
    mix_u, mix_p = (neg_beta * u).sum(dim=1), (neg_beta * p).sum(dim=1)
    u2, p2 = u[user_index, :], p[item_index, :]
    cl_u = user_beta * u + (1 - user_beta) * u2
    cl_p = item_beta * p + (1 - item_beta) * p2
    mix_q = item_beta * q + (1 - item_beta) * q[item_index, :]
    second = (1 - item_beta) * losses.get_InfoNCE_loss_all(u, p, mix_q, 1.0)
    user_ssl = user_beta * losses.get_InfoNCE_loss_all(u, cl_u, torch.cat([u2, mix_u]), t) \
        + (1 - user_beta) * losses.get_InfoNCE_loss_all(u2, cl_u, torch.cat([u, mix_u]), t)
    item_ssl = item_beta * losses.get_InfoNCE_loss_all(p, cl_p, torch.cat([p2, mix_p]), t) \
        + (1 - item_beta) * losses.get_InfoNCE_loss_all(p2, cl_p, torch.cat([p, mix_p]), t)
    return second, lam * (user_ssl + item_ssl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    args = ap.parse_args()
    from models.LightGCN import LightGCN
    from models.MixRec import MixRec

    root = tempfile.mkdtemp(prefix="idg_mixrec_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "MixRec.txt"), "MixRec")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K = 2048, 64, data.num_users, data.num_items, int(cfg["GCN_layer"])
    n = U + I
    reg, lam, t = float(cfg["reg_lambda"]), float(cfg["ssl_lambda"]), float(cfg["temperature"])
    abg = (float(cfg["alpha"]), float(cfg["beta"]), float(cfg["gamma"]))
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "steps": args.steps, "windows": args.windows}
    loss = torch.zeros(4, device="cuda")

    tools.set_seed(2024)
    m = MixRec(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    m.train()
    assert m.fused_step_available()

    tools.set_seed(2024)
    ma = MixRec(cfg, data, torch.device("cuda")).to("cuda")
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

    def device_draws():
        ub, ib, nu, up, ip = draw_mix(B, *abg)
        return ub, ib, nu.cuda(), up.cuda(), ip.cuda()

    named = [("fused", fused_step), ("autograd", autograd_step), ("lightgcn_fused", lightgcn_step)]
    if not args.skip_torch:
        # the reference's expressions (models/MixRec.py:44-60, 94-154) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        for e in (ue, ie):
            torch.nn.init.xavier_uniform_(e.weight, gain=1.)
        topt = torch.optim.Adam([ue.weight, ie.weight], lr=float(cfg["learn_rate"]))

        def torch_step(b):
            users, pos, neg = b
            x = torch.cat([ue.weight, ie.weight])
            layers = []
            for _ in range(K):
                x = torch.sparse.mm(A, x)
                layers.append(x)
            fu, fi = torch.split(torch.sum(torch.stack(layers, dim=1), dim=1), [U, I])
            u, p, q = fu[users], fi[pos], fi[neg]
            draws = device_draws()
            second, ssl = torch_terms(u, p, q, draws, t, lam)
            total = draws[1] * losses.get_bpr_loss(u, p, q) + second + reg * losses.get_reg_loss(ue(users), ie(pos), ie(neg)) + ssl
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

    # idg_mix_nce_f32 alone, and the same five terms in plain torch on the gathered rows
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n, d, device="cuda", generator=gen) * 0.1
    gX = torch.zeros_like(X)
    np.random.seed(1)
    torch.manual_seed(1)
    ub, ib, nu, up, ip = device_draws()
    ub, ib = 0.37, 0.61  # both halves of every term carry weight, whatever the Beta(0.1, 0.1) draw was
    ws = ops.mix_nce_workspace(B, d, X.device)
    pair = torch.zeros(2, device="cuda")
    users, pos, neg = batches[0]

    def kernel_fwd(_):
        ops.mix_nce_raw(X, U, users, pos, neg, up, ip, nu, ub, ib, t, lam, loss=pair, ws=ws)

    def kernel_fwd_bwd(_):
        ops.mix_nce_raw(X, U, users, pos, neg, up, ip, nu, ub, ib, t, lam, loss=pair, g_panel=gX, ws=ws)

    def rows_fwd(_):
        with torch.no_grad():
            torch_terms(X[users], X[U + pos], X[U + neg], (ub, ib, nu, up, ip), t, lam)

    Xg = X.clone().requires_grad_(True)

    def rows_fwd_bwd(_):
        second, ssl = torch_terms(Xg[users], Xg[U + pos], Xg[U + neg], (ub, ib, nu, up, ip), t, lam)
        Xg.grad = None
        (second + ssl).backward()

    alone = _alternate([("mix_nce_fwd", kernel_fwd), ("mix_nce_fwd_bwd", kernel_fwd_bwd), ("torch_terms_fwd", rows_fwd),
                        ("torch_terms_fwd_bwd", rows_fwd_bwd)], batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    Bp, dp = (B + 127) // 128 * 128, (d + 31) // 32 * 32
    product = 2.0 * Bp * Bp * dp
    for name, products in (("mix_nce_fwd", 3), ("mix_nce_fwd_bwd", 12), ("torch_terms_fwd", None), ("torch_terms_fwd_bwd", None)):
        med, lo, hi = alone[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        if products is not None:
            out[name + "_tflops"] = products * product / (med * 1e-3) / 1e12
    out["mix_nce_fwd_over_torch_terms"] = out["mix_nce_fwd_ms"] / out["torch_terms_fwd_ms"]
    out["mix_nce_fwd_bwd_over_torch_terms"] = out["mix_nce_fwd_bwd_ms"] / out["torch_terms_fwd_bwd_ms"]
    out["mix_nce_workspace_mb"] = ws.numel() / 2 ** 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
