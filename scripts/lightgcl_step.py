"""ms per LightGCL training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, GCN_layer = 2, svd_q = 5
(configure/LightGCL.txt), one JSON line: the fused step (idgrec_amd/lightgcl.py), the same model through forward() + autograd
+ ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm, the per-layer SVD views over all rows,
the two [B, N] score matrices, torch.optim.Adam), and the fused LightGCN step at the same shape — the yardstick of what the
propagation and BPR alone cost.  Every timed shape is warmed first; then the four are ALTERNATED: window w times --steps steps
of each in turn, and every figure is the median of the --windows windows, with the windows' min and max next to it.  All
share ONE set of SVD factors (torch.svd_lowrank at construction: not part of a step).

idg_svd_nce_f32 alone, both sides, on panels of the step's size: forward (losses only) and forward + backward, against the
same two terms per side in plain torch (forward, and forward + backward through autograd): ms, and TFLOP/s over the matrix
products the kernel actually performs on its zero-padded operands — 2 Bp Np dp per product, Bp and Np rounded up to 128, dp to
32; the loss-only call forms each score tile once (1 product per side), the gradient call forms it twice and multiplies it
into the rows twice (4 products per side).  The projection and the expansion alone, over the item rows: ms and GB/s over the
bytes they must move (the [n, d] panel and the [n, q] factor once, the expansion writing the panel once).

    python scripts/lightgcl_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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


def torch_side(g, table, ids, t):
    """The reference's two terms of one side (models/LightGCL.py:114-118) on plain torch: (log-sum-exp, clamped positive)."""
    neg = torch.log(torch.exp(g[ids] @ table.T / t).sum(1) + 1e-8).mean()
    pos = torch.clamp((table[ids] * g[ids]).sum(1) / t, -5.0, 5.0).mean()
    return neg, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    args = ap.parse_args()
    from models.LightGCL import LightGCL
    from models.LightGCN import LightGCN

    root = tempfile.mkdtemp(prefix="idg_lightgcl_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "LightGCL.txt"), "LightGCL")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048",
               GCN_layer="2", svd_q="5")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K, q = 2048, 64, data.num_users, data.num_items, int(cfg["GCN_layer"]), int(cfg["svd_q"])
    n = U + I
    reg, lam, t = float(cfg["reg_lambda"]), float(cfg["ssl_lambda"]), float(cfg["temperature"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "svd_q": q, "steps": args.steps,
           "windows": args.windows}
    loss = torch.zeros(3, device="cuda")

    tools.set_seed(2024)
    m = LightGCL(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    m.train()
    assert m.fused_step_available()
    factors = (m.svd_u, m.svd_s, m.svd_v)

    class Shared(LightGCL):
        factor_source = factors

    tools.set_seed(2024)
    ma = Shared(cfg, data, torch.device("cuda")).to("cuda")
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

    svd_u, s, svd_v = factors
    u_mul_s, v_mul_s = svd_u @ torch.diag(s), svd_v @ torch.diag(s)
    named = [("fused", fused_step), ("autograd", autograd_step), ("lightgcn_fused", lightgcn_step)]
    if not args.skip_torch:
        # the reference's expressions (models/LightGCL.py:58-124) as plain torch on the device
        R = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix_R(data)).coalesce().cuda()
        Rt = R.transpose(0, 1).coalesce()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        for e in (ue, ie):
            torch.nn.init.xavier_uniform_(e.weight, gain=1.)
        topt = torch.optim.Adam([ue.weight, ie.weight], lr=float(cfg["learn_rate"]))

        def torch_step(b):
            users, pos, neg = b
            eu, ei, gu, gi = [ue.weight], [ie.weight], [ue.weight], [ie.weight]
            for l in range(1, K + 1):
                zu, zi = torch.sparse.mm(R, ei[l - 1]), torch.sparse.mm(Rt, eu[l - 1])
                gu.append(u_mul_s @ (svd_v.T @ ei[l - 1]))
                gi.append(v_mul_s @ (svd_u.T @ eu[l - 1]))
                eu.append(zu)
                ei.append(zi)
            fu, fi = torch.stack(eu, dim=1).sum(dim=1), torch.stack(ei, dim=1).sum(dim=1)
            vu, vi = torch.stack(gu, dim=1).sum(dim=1), torch.stack(gi, dim=1).sum(dim=1)
            neg_u, pos_u = torch_side(vu, fu, users, t)
            neg_i, pos_i = torch_side(vi, fi, pos, t)
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg]) + reg * losses.get_reg_loss(ue(users), ie(pos), ie(neg)) \
                + lam * (-(pos_u + pos_i) + (neg_u + neg_i))
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

    # idg_svd_nce_f32 alone (both sides), and the same terms in plain torch
    gen = torch.Generator(device="cuda").manual_seed(1)
    F = torch.randn(n, d, device="cuda", generator=gen) * 0.1
    E = torch.randn(n, d, device="cuda", generator=gen) * 0.1
    Pi, Pu = torch.randn(q, d, device="cuda", generator=gen) * 0.1, torch.randn(q, d, device="cuda", generator=gen) * 0.1
    gF, gE, dP = torch.zeros_like(F), torch.zeros_like(E), torch.zeros_like(Pi)
    us, vs = u_mul_s.contiguous(), v_mul_s.contiguous()
    ws_u, ws_i = ops.svd_nce_workspace(B, U, d, q, F.device), ops.svd_nce_workspace(B, I, d, q, F.device)
    pair = torch.zeros(2, device="cuda")
    users, pos, _ = batches[0]

    def kernel_fwd(_):
        ops.svd_nce_raw(F, E, 0, U, us, Pi, users, t, loss=pair, ws=ws_u)
        ops.svd_nce_raw(F, E, U, I, vs, Pu, pos, t, loss=pair, ws=ws_i)

    def kernel_fwd_bwd(_):
        ops.svd_nce_raw(F, E, 0, U, us, Pi, users, t, loss=pair, g_final=gF, g_ego=gE, dP=dP, ws=ws_u)
        ops.svd_nce_raw(F, E, U, I, vs, Pu, pos, t, loss=pair, g_final=gF, g_ego=gE, dP=dP, ws=ws_i)

    def terms(Fx, Ex):
        g_u = Ex[:U][users] + us[users] @ Pi
        g_i = Ex[U:][pos] + vs[pos] @ Pu
        a = torch.log(torch.exp(g_u @ Fx[:U].T / t).sum(1) + 1e-8).mean() - torch.clamp((Fx[:U][users] * g_u).sum(1) / t, -5., 5.).mean()
        b = torch.log(torch.exp(g_i @ Fx[U:].T / t).sum(1) + 1e-8).mean() - torch.clamp((Fx[U:][pos] * g_i).sum(1) / t, -5., 5.).mean()
        return a + b

    def rows_fwd(_):
        with torch.no_grad():
            terms(F, E)

    Fg, Eg = F.clone().requires_grad_(True), E.clone().requires_grad_(True)

    def rows_fwd_bwd(_):
        Fg.grad = Eg.grad = None
        terms(Fg, Eg).backward()

    alone = _alternate([("svd_nce_fwd", kernel_fwd), ("svd_nce_fwd_bwd", kernel_fwd_bwd), ("torch_terms_fwd", rows_fwd),
                        ("torch_terms_fwd_bwd", rows_fwd_bwd)], batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    up128 = lambda x: (x + 127) // 128 * 128  # noqa: E731
    product = 2.0 * up128(B) * (up128(U) + up128(I)) * ((d + 31) // 32 * 32)
    for name, products in (("svd_nce_fwd", 1), ("svd_nce_fwd_bwd", 4), ("torch_terms_fwd", None), ("torch_terms_fwd_bwd", None)):
        med, lo, hi = alone[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        if products is not None:
            out[name + "_tflops"] = products * product / (med * 1e-3) / 1e12
    out["svd_nce_fwd_over_torch_terms"] = out["svd_nce_fwd_ms"] / out["torch_terms_fwd_ms"]
    out["svd_nce_fwd_bwd_over_torch_terms"] = out["svd_nce_fwd_bwd_ms"] / out["torch_terms_fwd_bwd_ms"]
    out["svd_nce_workspace_mb"] = (ws_u.numel() + ws_i.numel()) / 2 ** 20

    # the projection and the expansion alone, over the item rows
    Y = torch.empty(I, d, device="cuda")

    def project(_):
        ops.lowrank_project_raw(svd_v, F[U:], out=dP)

    def expand(_):
        ops.lowrank_expand_raw(svd_v, Pi, Y=Y)

    lr = _alternate([("lowrank_project", project), ("lowrank_expand", expand)], batches, max(args.steps, 50), max(args.warmup, 10),
                    args.windows)
    moved = 4.0 * I * (d + q)
    for name in ("lowrank_project", "lowrank_expand"):
        med, lo, hi = lr[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        out[name + "_gbs"] = moved / (med * 1e-3) / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
