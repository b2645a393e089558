"""ms per LR-GCCF training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, K = 3
(configure/GCCF.txt), one JSON line: the fused step (idgrec_amd/gccf.py), the same model through forward() + autograd +
ops.Adam, the reference's expressions as plain torch on the device (torch.sparse.mm, torch.matmul, nn.Dropout,
torch.optim.Adam), and the fused NgcfEngine step at the same shape — the yardstick: per layer LR-GCCF stages one panel where
NGCF stages two, issues half the MFMAs, reads one panel fewer in its backward and has no g_ego product.  Every timed shape is
warmed first; then the four are ALTERNATED: window w times --steps steps of each in turn, and every figure is the median of
the --windows windows, with the windows' min and max next to it.

Each of the two layer kernels alone, on panels of the step's size: ms, effective GB/s over its minimal traffic (forward:
read side, write E; backward: read gE and side, write g_side) and TFLOP/s over 2 n d^2 per product (forward: one product;
backward: two).  The panels (18 MB each) live in the Infinity Cache, so the GB/s are not a share of the HBM peak.

    python scripts/gccf_step.py [--steps 20] [--warmup 5] [--windows 5] [--skip-torch]
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
    from models.GCCF import GCCF
    from models.NGCF import NGCF

    root = tempfile.mkdtemp(prefix="idg_gccf_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "GCCF.txt"), "GCCF")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I, K = 2048, 64, data.num_users, data.num_items, int(cfg["GCN_layer"])
    n = U + I
    drop = eval(cfg["mess_drop_prob"])
    np.random.seed(0)
    tri = torch.from_numpy(data.sample_data_to_train_all()[:16 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(16)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "layers": K, "mess_drop_prob": drop, "steps": args.steps,
           "windows": args.windows}
    loss = torch.zeros(2, device="cuda")

    tools.set_seed(2024)
    m = GCCF(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    m.train()
    assert m.fused_step_available()

    # the same model once more for the autograd path: the fused step keeps its small tensors in the engine's flat buffer
    tools.set_seed(2024)
    ma = GCCF(cfg, data, torch.device("cuda")).to("cuda")
    aopt = ops.Adam(ma.parameters(), lr=float(cfg["learn_rate"]))
    ma.train()

    def fused_step(b):
        assert m.fused_train_step(*b, loss, opt)

    def autograd_step(b):
        ll = ma(*b)
        aopt.zero_grad()
        sum(ll).backward()
        aopt.step()

    ncfg = tools.read_configuration(os.path.join(ROOT, "configure", "NGCF.txt"), "NGCF")
    ncfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048",
                GCN_layer=str(K), layer_size=str([d] * K), mess_drop_prob=str(drop), node_dropout="False")
    tools.set_seed(2024)
    ng = NGCF(ncfg, data, torch.device("cuda")).to("cuda")
    nopt = ops.Adam(ng.parameters(), lr=float(ncfg["learn_rate"]))
    ng.train()
    assert ng.fused_step_available()

    def ngcf_step(b):
        assert ng.fused_train_step(*b, loss, nopt)

    named = [("fused", fused_step), ("autograd", autograd_step), ("ngcf_fused", ngcf_step)]
    if not args.skip_torch:
        # the reference's expressions (models/GCCF.py:60-110) as plain torch on the device
        A = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix_with_self(data)).coalesce().cuda()
        tools.set_seed(2024)
        ue, ie = torch.nn.Embedding(U, d).cuda(), torch.nn.Embedding(I, d).cuda()
        torch.nn.init.xavier_uniform_(ue.weight, gain=1)
        torch.nn.init.xavier_uniform_(ie.weight, gain=1)
        Ws = [torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(d, d, device="cuda"))) for _ in range(K)]
        bs = [torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(1, d, device="cuda"))) for _ in range(K)]
        topt = torch.optim.Adam(list(ue.parameters()) + list(ie.parameters()) + Ws + bs, lr=float(cfg["learn_rate"]))

        def torch_step(b):
            users, pos, neg = b
            ego = torch.cat([ue.weight, ie.weight])
            layers = [ego]
            for l in range(K):
                ego = torch.nn.Dropout(drop[l])(torch.matmul(torch.sparse.mm(A, ego), Ws[l]) + bs[l])
                layers.append(ego)
            fu, fi = torch.split(torch.cat(layers, dim=1), [U, I])
            total = losses.get_bpr_loss(fu[users], fi[pos], fi[neg]) + m.reg_lambda * losses.get_reg_loss(ie(pos), ie(neg))
            topt.zero_grad()
            total.backward()
            topt.step()

        named.append(("torch", torch_step))

    for name, (med, lo, hi) in _alternate(named, batches, args.steps, args.warmup, args.windows).items():
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
    out["fused_over_ngcf_fused"] = out["fused_ms"] / out["ngcf_fused_ms"]
    out["fused_over_autograd"] = out["fused_ms"] / out["autograd_ms"]
    if not args.skip_torch:
        out["fused_over_torch"] = out["fused_ms"] / out["torch_ms"]

    # the two layer kernels alone, on panels of the step's size
    gen = torch.Generator(device="cuda").manual_seed(1)
    side, gE = (torch.randn(n, d, device="cuda", generator=gen) for _ in range(2))
    W, b = torch.randn(d, d, device="cuda", generator=gen) * 0.1, torch.randn(d, device="cuda", generator=gen) * 0.1
    E, g_side, w_grads = torch.empty_like(side), torch.empty_like(side), torch.empty(d * d + d, device="cuda")
    panel, flop = n * d * 4, 2.0 * n * d * d
    alone = _alternate([("layer_fwd", lambda _: ops.gccf_layer_fwd_raw(side, W, b, drop[0], 1234, 7, E)),
                        ("layer_bwd", lambda _: ops.gccf_layer_bwd_raw(gE, None, d, None, side, W, drop[0], 1234, 7, g_side, w_grads))],
                       batches, max(args.steps, 50), max(args.warmup, 10), args.windows)
    for name, traffic, products in (("layer_fwd", 2 * panel, 1), ("layer_bwd", 3 * panel, 2)):
        med, lo, hi = alone[name]
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = med, lo, hi
        out[name + "_gbs"] = traffic / (med * 1e-3) / 1e9
        out[name + "_tflops"] = products * flop / (med * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
