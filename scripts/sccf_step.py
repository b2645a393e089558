"""ms per SCCF training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, both encoders (MF, and
LightGCN with GCN_layer = 3), one JSON line.  Per encoder, in the same run: the fused step (PropagationEngine.sccf), the same
model through forward() + autograd + ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm,
two torch.unique calls, the [Nu, Ni] score matrix and count outer product, torch.optim.Adam), and the fused DirectAU step of
the same encoder — the chain that differs from SCCF's in the loss call only.  Every timed shape is warmed first; then they are
ALTERNATED: window w times --steps steps of each in turn, and every figure is the median of the --windows windows, with the
windows' min and max next to it.

idg_sccf_loss_f32 alone on a panel of the step's size, the losses only and with gradients, against the same two terms in
plain torch on the gathered rows (unique included; forward, and forward + backward through autograd): ms, and TFLOP/s over
the matrix products the kernel performs on its zero-padded operands — 2 Bp^2 dp per product, Bp = B rounded up to 128, dp = d
rounded up to 32; one product for the losses, three with gradients — and the workspace size.

    python scripts/sccf_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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


def torch_terms(fu, fi, users, pos, t):
    """The reference's two terms (models/SCCF.py:60-80) on the encoder's output, plain torch."""
    u_idx, u_counts = torch.unique(users, return_counts=True)
    i_idx, i_counts = torch.unique(pos, return_counts=True)
    u_counts, i_counts = u_counts.reshape(-1, 1).float(), i_counts.reshape(-1, 1).float()
    a, b = F.normalize(fu[users], dim=-1), F.normalize(fi[pos], dim=-1)
    ip = (a * b).sum(dim=1)
    up = ((ip / t).exp() + (ip ** 2 / t).exp()).log().mean()
    a, b = F.normalize(fu[u_idx], dim=-1), F.normalize(fi[i_idx], dim=-1)
    sim = a @ b.T
    score = (sim / t).exp() + (sim ** 2 / t).exp()
    down = (score * (u_counts @ i_counts.T)).mean().log()
    return -up, down


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    args = ap.parse_args()
    from models.DirectAU import DirectAU
    from models.SCCF import SCCF

    root = tempfile.mkdtemp(prefix="idg_sccf_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    base = dict(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048", GCN_layer="3")
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "SCCF.txt"), "SCCF")
    cfg.update(base)
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K = 2048, 64, data.num_users, data.num_items, 3
    n = U + I
    t = float(cfg["temperature"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "temperature": t, "steps": args.steps,
           "windows": args.windows}
    A = None
    for enc, tag in (("MF", "mf"), ("LightGCN", "gcn")):
        loss, loss3 = torch.zeros(2, device="cuda"), torch.zeros(3, device="cuda")
        models = []
        for _ in range(2):
            tools.set_seed(2024)
            m = SCCF(dict(cfg, encoder=enc), data, torch.device("cuda")).to("cuda")
            m.train()
            models.append((m, ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))))
        (m, opt), (ma, aopt) = models
        assert m.fused_step_available()
        acfg = tools.read_configuration(os.path.join(ROOT, "configure", "DirectAU.txt"), "DirectAU")
        acfg.update(base, encoder=enc)
        tools.set_seed(2024)
        au = DirectAU(acfg, data, torch.device("cuda")).to("cuda")
        au.train()
        auopt = ops.Adam(au.parameters(), lr=float(acfg["learn_rate"]))
        assert au.fused_step_available()

        def fused_step(b, m=m, opt=opt, loss=loss):
            assert m.fused_train_step(*b, loss, opt)

        def autograd_step(b, ma=ma, aopt=aopt):
            ll = ma(*b)
            aopt.zero_grad()
            sum(ll).backward()
            aopt.step()

        def directau_step(b, au=au, auopt=auopt, loss3=loss3):
            assert au.fused_train_step(*b, loss3, auopt)

        named = [("fused", fused_step), ("autograd", autograd_step), ("directau_fused", directau_step)]
        if not args.skip_torch:
            if A is None and enc != "MF":
                A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix(data)).coalesce().cuda()
            tools.set_seed(2024)
            ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
            for e in (ue, ie):
                torch.nn.init.xavier_uniform_(e.weight, gain=1.)
            topt = torch.optim.Adam([ue.weight, ie.weight], lr=float(cfg["learn_rate"]))

            def torch_step(b, enc=enc, ue=ue, ie=ie, topt=topt):
                users, pos, _ = b
                if enc == "MF":
                    fu, fi = ue.weight, ie.weight
                else:
                    x = torch.cat([ue.weight, ie.weight])
                    layers = [x]
                    for _ in range(K):
                        x = torch.sparse.mm(A, x)
                        layers.append(x)
                    fu, fi = torch.split(torch.mean(torch.stack(layers, dim=1), dim=1), [U, I])
                topt.zero_grad()
                sum(torch_terms(fu, fi, users, pos, t)).backward()
                topt.step()

            named.append(("torch", torch_step))
        for name, (med, lo, hi) in _alternate(named, batches, args.steps, args.warmup, args.windows).items():
            out["%s_%s_ms" % (tag, name)], out["%s_%s_ms_min" % (tag, name)], out["%s_%s_ms_max" % (tag, name)] = med, lo, hi
        out[tag + "_fused_over_autograd"] = out[tag + "_fused_ms"] / out[tag + "_autograd_ms"]
        out[tag + "_fused_over_directau_fused"] = out[tag + "_fused_ms"] / out[tag + "_directau_fused_ms"]
        if not args.skip_torch:
            out[tag + "_fused_over_torch"] = out[tag + "_fused_ms"] / out[tag + "_torch_ms"]
        del models, m, ma, au

    # idg_sccf_loss_f32 alone, and the same two terms in plain torch on the gathered rows
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n, d, device="cuda", generator=gen) * 0.1
    gX = torch.zeros_like(X)
    ws = ops.sccf_workspace(B, d, X.device)
    pair = torch.zeros(2, device="cuda")
    users, pos, _ = batches[0]

    def kernel_loss(_):
        ops.sccf_loss_raw(X, users, pos, U, t, loss=pair, ws=ws)

    def kernel_loss_grad(_):
        ops.sccf_loss_raw(X, users, pos, U, t, gX, loss=pair, ws=ws)

    def rows_fwd(_):
        with torch.no_grad():
            torch_terms(X[:U], X[U:], users, pos, t)

    Xg = X.clone().requires_grad_(True)

    def rows_fwd_bwd(_):
        Xg.grad = None
        sum(torch_terms(Xg[:U], Xg[U:], users, pos, t)).backward()

    alone = _alternate([("sccf_loss", kernel_loss), ("sccf_loss_grad", kernel_loss_grad), ("torch_terms_fwd", rows_fwd),
                        ("torch_terms_fwd_bwd", rows_fwd_bwd)], batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    Bp, dp = (B + 127) // 128 * 128, (d + 31) // 32 * 32
    product = 2.0 * Bp * Bp * dp
    for name, products in (("sccf_loss", 1), ("sccf_loss_grad", 3), ("torch_terms_fwd", None), ("torch_terms_fwd_bwd", None)):
        med, lo, hi = alone[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        if products is not None:
            out[name + "_tflops"] = products * product / (med * 1e-3) / 1e12
    out["sccf_loss_over_torch_terms"] = out["sccf_loss_ms"] / out["torch_terms_fwd_ms"]
    out["sccf_loss_grad_over_torch_terms"] = out["sccf_loss_grad_ms"] / out["torch_terms_fwd_bwd_ms"]
    out["sccf_workspace_mb"] = ws.numel() / 2 ** 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
