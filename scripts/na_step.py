"""ms per LightCCF / LightCSCF training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 4096 (the models'
own batch size), both models with both encoders (MF, and LightGCN with GCN_layer = 3), one JSON line.  Per model and encoder,
in the same run: the fused step (PropagationEngine.na), the same model through forward() + autograd + ops.Adam, the
reference's expressions as plain torch on the device (torch.sparse.mm, two [B, B] matmuls added, torch.optim.Adam), and the
fused LightGCN step at the same batch size.  Every timed shape is warmed first; then they are ALTERNATED: window w times
--steps steps of each in turn, and every figure is the median of the --windows windows, with the windows' min and max next
to it.

idg_na_nce_f32 alone (LightCCF's form and LightCSCF's) on a panel of the step's size, the loss only and with gradients,
against the same term in plain torch on the gathered rows (forward, and forward + backward through autograd): ms, and
TFLOP/s over the double-precision matrix products the kernel performs on its zero-padded operands — 2 Bp^2 dp per product,
Bp = B rounded up to 64, dp = d rounded up to 32; one product for the loss, five with gradients (the scores three times, P . C
and P^T . A) — and the workspace size.

    python scripts/na_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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
import torch.nn.functional as F  # noqa: E402

import idgrec_amd.synth as S  # noqa: E402
import utility.utility_data.data_graph as data_graph  # noqa: E402
import utility.utility_data.data_loader as data_loader  # noqa: E402
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


def torch_term(ue, pe, t, margin):
    """The reference's term (models/LightCCF.py:81-94, models/LightCSCF.py:93-104) on the gathered rows, plain torch."""
    a, b = F.normalize(ue, dim=1), F.normalize(pe, dim=1)
    sim = (a * b).sum(dim=-1)
    total = torch.matmul(a, b.transpose(0, 1)) + torch.matmul(a, a.transpose(0, 1))
    if margin is None:
        pos_score, total = torch.exp(sim / t), torch.exp(total / t).sum(dim=1)
    else:
        pos_score = torch.exp(sim / t) + torch.exp(torch.relu(sim - margin) / t)
        total = (torch.exp(total / t) + torch.exp(torch.relu(total - margin) / t)).sum(dim=1)
    return torch.mean(-torch.log(pos_score / total + 10e-6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    args = ap.parse_args()
    from models.LightCCF import LightCCF
    from models.LightCSCF import LightCSCF
    from models.LightGCN import LightGCN

    root = tempfile.mkdtemp(prefix="idg_na_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    base = dict(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="4096", GCN_layer="3")
    cfgs = {}
    for name in ("LightCCF", "LightCSCF", "LightGCN"):
        cfgs[name] = tools.read_configuration(os.path.join(ROOT, "configure", name + ".txt"), name)
        cfgs[name].update(base)
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfgs["LightCCF"])
    B, d, U, I, K = 4096, 64, data.num_users, data.num_items, 3
    n = U + I
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "steps": args.steps, "windows": args.windows}
    tools.set_seed(2024)
    lg = LightGCN(cfgs["LightGCN"], data, torch.device("cuda")).to("cuda")
    lg.train()
    lgopt = ops.Adam(lg.parameters(), lr=float(cfgs["LightGCN"]["learn_rate"]))
    lgloss = torch.zeros(2, device="cuda")
    assert lg.fused_step_available()

    def lightgcn_step(b):
        assert lg.fused_train_step(*b, lgloss, lgopt)

    A = None
    for cls, name, short in ((LightCCF, "LightCCF", "ccf"), (LightCSCF, "LightCSCF", "cscf")):
        cfg = cfgs[name]
        t = float(cfg["temperature"])
        if name == "LightCCF":
            reg, weight, margin = float(cfg["reg_lambda"]), float(cfg["ssl_lambda"]), None
        else:
            reg, weight, margin = float(cfg["lambda_reg"]), float(cfg["lambda_gamma"]), float(cfg["lambda_margin"])
        out[short + "_temperature"] = t
        for enc, etag in (("MF", "mf"), ("LightGCN", "gcn")):
            tag = "%s_%s" % (short, etag)
            with_bpr = not (name == "LightCSCF" and enc != "MF")
            models = []
            for _ in range(2):
                tools.set_seed(2024)
                m = cls(dict(cfg, encoder=enc), data, torch.device("cuda")).to("cuda")
                m.train()
                models.append((m, ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))))
            (m, opt), (ma, aopt) = models
            assert m.fused_step_available()
            loss = torch.zeros(m.n_fused_losses, device="cuda")

            def fused_step(b, m=m, opt=opt, loss=loss):
                assert m.fused_train_step(*b, loss, opt)

            def autograd_step(b, ma=ma, aopt=aopt):
                ll = ma(*b)
                aopt.zero_grad()
                sum(ll).backward()
                aopt.step()

            named = [("fused", fused_step), ("autograd", autograd_step), ("lightgcn_fused", lightgcn_step)]
            if not args.skip_torch:
                if A is None and enc != "MF":
                    A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
                tools.set_seed(2024)
                ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
                for e in (ue, ie):
                    torch.nn.init.xavier_uniform_(e.weight, gain=1.)
                topt = torch.optim.Adam([ue.weight, ie.weight], lr=float(cfg["learn_rate"]))

                def torch_step(b, enc=enc, ue=ue, ie=ie, topt=topt, t=t, reg=reg, weight=weight, margin=margin, with_bpr=with_bpr):
                    users, pos, neg = b
                    if enc == "MF":
                        fu, fi = ue.weight, ie.weight
                    else:
                        x = torch.cat([ue.weight, ie.weight])
                        layers = [x]
                        for _ in range(K):
                            x = torch.sparse.mm(A, x)
                            layers.append(x)
                        fu, fi = torch.split(torch.mean(torch.stack(layers, dim=1), dim=1), [U, I])
                    u, p, q = fu[users], fi[pos], fi[neg]
                    ll = [reg * sum(0.5 * e.norm(2).pow(2) / float(e.shape[0]) for e in (ue(users), ie(pos), ie(neg))),
                          weight * torch_term(u, p, t, margin)]
                    if with_bpr:
                        ll.append(torch.mean(-torch.log(torch.sigmoid((u * p).sum(1) - (u * q).sum(1)) + 10e-8)))
                    topt.zero_grad()
                    sum(ll).backward()
                    topt.step()

                named.append(("torch", torch_step))
            for nm, (med, lo, hi) in _alternate(named, batches, args.steps, args.warmup, args.windows).items():
                out["%s_%s_ms" % (tag, nm)], out["%s_%s_ms_min" % (tag, nm)], out["%s_%s_ms_max" % (tag, nm)] = med, lo, hi
            out[tag + "_fused_over_autograd"] = out[tag + "_fused_ms"] / out[tag + "_autograd_ms"]
            out[tag + "_fused_over_lightgcn_fused"] = out[tag + "_fused_ms"] / out[tag + "_lightgcn_fused_ms"]
            if not args.skip_torch:
                out[tag + "_fused_over_torch"] = out[tag + "_fused_ms"] / out[tag + "_torch_ms"]
            del models, m, ma

    # idg_na_nce_f32 alone, and the same term in plain torch on the gathered rows
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n, d, device="cuda", generator=gen) * 0.1
    gX = torch.zeros_like(X)
    ws = ops.na_nce_workspace(B, d, X.device)
    one = torch.zeros(1, device="cuda")
    users, pos, _ = batches[0]
    Xg = X.clone().requires_grad_(True)
    Bp, dp = (B + 63) // 64 * 64, (d + 31) // 32 * 32
    product = 2.0 * Bp * Bp * dp
    for short, t, margin in (("ccf", float(cfgs["LightCCF"]["temperature"]), None),
                             ("cscf", float(cfgs["LightCSCF"]["temperature"]), float(cfgs["LightCSCF"]["lambda_margin"]))):
        def kernel_loss(_, t=t, margin=margin):
            ops.na_nce_loss_raw(X, users, pos, U, t, margin, 1.0, loss=one, ws=ws)

        def kernel_loss_grad(_, t=t, margin=margin):
            ops.na_nce_loss_raw(X, users, pos, U, t, margin, 1.0, gX, loss=one, ws=ws)

        def rows_fwd(_, t=t, margin=margin):
            with torch.no_grad():
                torch_term(X[users], X[U + pos], t, margin)

        def rows_fwd_bwd(_, t=t, margin=margin):
            Xg.grad = None
            torch_term(Xg[users], Xg[U + pos], t, margin).backward()

        alone = _alternate([("na_nce_loss", kernel_loss), ("na_nce_loss_grad", kernel_loss_grad), ("torch_term_fwd", rows_fwd),
                            ("torch_term_fwd_bwd", rows_fwd_bwd)], batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
        for nm, products in (("na_nce_loss", 1), ("na_nce_loss_grad", 5), ("torch_term_fwd", None), ("torch_term_fwd_bwd", None)):
            med, lo, hi = alone[nm]
            key = "%s_%s" % (short, nm)
            out[key + "_ms"], out[key + "_ms_min"], out[key + "_ms_max"] = med, lo, hi
            if products is not None:
                out[key + "_fp64_tflops"] = products * product / (med * 1e-3) / 1e12
        out[short + "_na_nce_loss_over_torch_term"] = out[short + "_na_nce_loss_ms"] / out[short + "_torch_term_fwd_ms"]
        out[short + "_na_nce_loss_grad_over_torch_term"] = out[short + "_na_nce_loss_grad_ms"] / out[short + "_torch_term_fwd_bwd_ms"]
    out["na_nce_workspace_mb"] = ws.numel() / 2 ** 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
