"""ms per CVGA training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 1024, one JSON line: the fused
step (encoder rows, head, idg_multinomial_nll_f32, head backward, transposed SpMM, Adam on the four tensors), the same
model through forward() + autograd + torch.optim.Adam, and the reference's own expressions as plain torch on the device
(sparse addmm over all U users, dense x built on the host and copied, materialised log_softmax), and the decoder call
idg_multinomial_nll_f32 alone (loss and the three gradients) with its TFLOP/s.  Device-event timing after a warm-up.
--skip-torch leaves out the plain-torch composition; --fused-only times the fused step and nothing else (what a kernel
trace of the fused step is taken from: profiles/cvga/).

    python scripts/cvga_step.py [--steps 50] [--warmup 10] [--skip-torch] [--fused-only]
"""
import argparse
import json
import os
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


def _time(step, batches, steps, warmup):
    for i in range(warmup):
        step(batches[i % len(batches)])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        step(batches[i % len(batches)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the plain-torch composition")
    ap.add_argument("--fused-only", action="store_true", help="time the fused step only")
    args = ap.parse_args()
    from models.CVGA import CVGA

    root = tempfile.mkdtemp(prefix="idg_cvga_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "CVGA.txt"), "CVGA")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="1024")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B, d, U, I = 1024, 64, data.num_users, data.num_items
    order = np.random.default_rng(0).permutation(U)
    nb = U // B
    batches = [torch.from_numpy(order[i * B:(i + 1) * B]).cuda() for i in range(nb)]
    out = {"shape": "yelp2018", "d": d, "B": B, "U": U, "I": I, "steps": args.steps}

    tools.set_seed(2024)
    m = CVGA(cfg, data, torch.device("cuda")).to("cuda")
    opt = torch.optim.Adam(m.parameters(), lr=0.001)
    loss = torch.zeros(2, device="cuda")
    m.train()
    out["fused_ms"] = _time(lambda b: m.fused_train_step(b, loss, opt), batches, args.steps, args.warmup)
    if args.fused_only:
        print(json.dumps(out))
        return

    def autograd_step(b):
        ll = m(b, None)
        opt.zero_grad()
        sum(ll).backward()
        opt.step()

    out["autograd_ms"] = _time(autograd_step, batches, args.steps, args.warmup)

    # the decoder call alone: (4 x 2 B I d) FLOP of logits (twice), dZ and dW
    z = torch.randn(B, d, device="cuda")
    W, c = m.p_layers[0].weight.data, m.p_layers[0].bias.data
    ip, ix, iv = m._train_csr()
    g = (torch.empty_like(z), torch.empty_like(W), torch.empty_like(c))
    ws = ops.multinomial_nll_workspace(B, I, d, "cuda")
    out["decoder_ms"] = _time(lambda b: ops.multinomial_nll_raw(z, W, c, b, ip, ix, iv, loss=loss[:1], gZ=g[0], gW=g[1],
                                                                gc=g[2], ws=ws), batches, args.steps, args.warmup)
    out["decoder_tflops"] = 4 * 2 * B * I * d / (out["decoder_ms"] * 1e-3) / 1e12
    out["decoder_share_of_fp32_matrix_peak"] = out["decoder_tflops"] / 157.3

    if not args.skip_torch:
        # the reference's expressions (models/CVGA.py:40-75, 130-150) as plain torch on the device
        R = tools.convert_sp_mat_to_sp_tensor(data_graph.sparse_adjacency_matrix_R(data)).coalesce().cuda()
        tools.set_seed(2024)
        lq, lp = torch.nn.Linear(I, 2 * d).cuda(), torch.nn.Linear(d, I).cuda()
        drop = torch.nn.Dropout(0.3)
        topt = torch.optim.Adam(list(lq.parameters()) + list(lp.parameters()), lr=0.001)
        train = data.user_item_net

        def torch_step(b):
            users = b.cpu().numpy()
            x = torch.FloatTensor(train[users].toarray()).to("cuda")
            h = drop(torch.sparse.addmm(lq.bias.unsqueeze(0).expand(U, -1), R, lq.weight.t()))
            mu, logvar = h[:, :d], h[:, d:]
            zz = torch.randn_like(mu).mul(torch.exp(0.5 * logvar)) + mu
            recon = lp(zz[b])
            bce, kld = losses.get_ELBO_loss(recon, x, mu[b], logvar[b], 1.0)
            topt.zero_grad()
            (bce + kld).backward()
            topt.step()

        out["torch_ms"] = _time(torch_step, batches, max(5, args.steps // 5), max(2, args.warmup // 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
